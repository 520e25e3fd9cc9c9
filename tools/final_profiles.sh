# refresh the judged artefacts: MFMA counters + PMC traffic (tools/pmc.py), rocprofv3 kernel stats of the same command, bench line
# usage (GPU box): bash tools/final_profiles.sh r02 [extra bench args]
export TMPDIR=/tmp; R=$GRAFT_REPO_ROOT; T=${1:-r02}; shift
OUT=${OUT:-$R/profile_out}; mkdir -p $OUT
cd $R && python3 tools/pmc.py $T "$@" > $OUT/${T}_pmc.log 2>&1; tail -22 $OUT/${T}_pmc.log
cd /tmp && rm -rf $OUT/stats && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -- python3 $R/bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-profile --no-pmc --no-extras "$@" > $OUT/stats.log 2>&1
cp $(find $OUT/stats -name '*kernel_stats.csv' | head -1) $OUT/${T}_bench_kernel_stats.csv
cd $R && python3 bench.py --full "$@" > $OUT/${T}_bench.json.log 2>$OUT/${T}_bench.err; tail -1 $OUT/${T}_bench.json.log | cut -c1-3000
