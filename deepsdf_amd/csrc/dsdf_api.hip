// dsdf_api.hip -- the C ABI of libdsdf_hip.so (include/dsdf.h): workspace planning + launch sequencing.
// No device allocation, no synchronisation, no global mutable state (thread-local error string only).
#include "../../include/dsdf.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <stdlib.h>

#include <algorithm>
#include <atomic>
#ifdef DSDF_LAB
#include <vector>
#endif

#include "dwstream.hpp"
#include "sample.hpp"
#include "fused.hpp"
#include "fused_bf16x8.hpp"
#include "gemm.hpp"
#include "kernels.hpp"
#include "mcubes.hpp"
#include "meshsdf.hpp"
#include "msgrid.hpp"
#include "msdiff.hpp"
#include "voldiff.hpp"
#include "pointset.hpp"
#include "meshtopo.hpp"
#include "sparsegrid.hpp"
#include "tetmesh.hpp"
#include "fem.hpp"

using namespace dsdf;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_OK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return fail(DSDF_E_LAUNCH, "%s failed: %s", #expr, hipGetErrorString(e_));   \
  } while (0)
#define LAUNCH_OK(name)                                                                                \
  do {                                                                                                 \
    hipError_t e_ = hipGetLastError();                                                                 \
    if (e_ != hipSuccess) return fail(DSDF_E_LAUNCH, "launch of %s failed: %s", name, hipGetErrorString(e_)); \
  } while (0)
#define TRY(expr)            \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != 0) return rc_; \
  } while (0)

// ---- optional per-kernel-class timing with HIP events (diagnostics; off by default) ----------------
struct Prof {
  bool on = false;
  static constexpr int NCLS = DSDF_PROF_CLASSES, POOL = 8192;
  hipEvent_t ev[POOL][2];
  int cls[POOL];
  int created = 0, used = 0;
  double flops[NCLS] = {0};
};
thread_local Prof g_prof;

struct ProfScope {
  int slot = -1;
  hipStream_t st;
  ProfScope(int cls, double flops, hipStream_t s) : st(s) {
    Prof& P = g_prof;
    if (!P.on || P.used >= Prof::POOL) return;
    if (P.used >= P.created) {
      if (hipEventCreate(&P.ev[P.created][0]) != hipSuccess || hipEventCreate(&P.ev[P.created][1]) != hipSuccess) return;
      ++P.created;
    }
    slot = P.used++;
    P.cls[slot] = cls;
    P.flops[cls] += flops;
    (void)hipEventRecord(P.ev[slot][0], st);
  }
  ~ProfScope() {
    if (slot >= 0) (void)hipEventRecord(g_prof.ev[slot][1], st);
  }
};

inline int64_t rup(int64_t x, int64_t m) { return (x + m - 1) / m * m; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

constexpr int NSPLIT_MAX = 32;     // split-K factor of the dW GEMMs
constexpr int LAST_BLOCKS_MAX = 1024;
constexpr int LAT_SLICES_MAX = 8;   // partial copies of the per-segment latent gradient (SegLatArgs.nslice)
constexpr int LAST_GROUPS = 16;    // second-stage partial groups of the last-layer reduction
constexpr int LN_BLOCKS = 256;     // LayerNorm backward: fixed grid = fixed summation order of its column partials

int validate(const DsdfNet* n) {
  if (!n) return fail(DSDF_E_INVALID, "net is NULL");
  if (n->n_layers < 2 || n->n_layers > DSDF_MAX_LAYERS) return fail(DSDF_E_INVALID, "n_layers %d out of range", n->n_layers);
  const int W0 = n->latent_size + n->geom_dim;
  if (n->latent_size < 0 || n->geom_dim < 1) return fail(DSDF_E_INVALID, "bad latent_size/geom_dim");
  // the d/d(xyz) scratch of an xyz_in_all net (module_backward with d_input, the tangent pass) is laid out [N][4]
  if (n->xyz_in_all && n->geom_dim > 4) return fail(DSDF_E_INVALID, "xyz_in_all needs geom_dim <= 4 (got %d)", n->geom_dim);
  if (n->in_dim[0] != W0) return fail(DSDF_E_INVALID, "in_dim[0] %d != latent_size+geom_dim %d", n->in_dim[0], W0);
  if (n->out_dim[n->n_layers - 1] != 1) return fail(DSDF_E_INVALID, "last layer must have out_dim 1");
  if (n->skip_mask & 1u) return fail(DSDF_E_INVALID, "latent_in may not contain layer 0");
  if (n->skip_mask >> n->n_layers) return fail(DSDF_E_INVALID, "skip_mask names a layer >= n_layers");
  if (__builtin_popcount(n->skip_mask) > 1) return fail(DSDF_E_INVALID, "at most one latent_in layer is supported");
  for (int l = 0; l < n->n_layers; ++l) {
    if (n->in_dim[l] < 1 || n->out_dim[l] < 1 || n->in_dim[l] > 2048 || n->out_dim[l] > 65536)
      return fail(DSDF_E_INVALID, "layer %d: unsupported size %d -> %d", l, n->in_dim[l], n->out_dim[l]);
    if (n->fwd_bf16 && (n->in_dim[l] > 512 || (l < n->n_layers - 1 && n->out_dim[l] > 512)))
      return fail(DSDF_E_INVALID, "fwd_bf16 needs every layer width <= 512 (layer %d: %d -> %d)", l, n->in_dim[l], n->out_dim[l]);
    if (l > 0) {
      const int expect = n->out_dim[l - 1] + ((n->skip_mask >> l) & 1 ? W0 : (n->xyz_in_all ? n->geom_dim : 0));
      if (n->in_dim[l] != expect) return fail(DSDF_E_INVALID, "layer %d: in_dim %d != %d", l, n->in_dim[l], expect);
    }
  }
  if ((n->latent_dropout || n->xyz_in_all || n->ln_param_mask) && n->fwd_bf16)
    return fail(DSDF_E_INVALID, "fwd_bf16 is not available with latent_dropout / xyz_in_all / LayerNorm");
  if (n->fwd_bf16 && ((n->skip_mask >> (n->n_layers - 1)) & 1))   // the bf16 kernels' output layer is a dot product over the activations only
    return fail(DSDF_E_INVALID, "fwd_bf16 is not available when latent_in names the output layer");
  if (n->gemm_split) {
    if (n->latent_dropout || n->xyz_in_all || n->ln_param_mask)
      return fail(DSDF_E_INVALID, "gemm_split is not available with latent_dropout / xyz_in_all / LayerNorm");
    for (int l = 0; l < n->n_layers; ++l)
      if (n->in_dim[l] > 512 || (l < n->n_layers - 1 && n->out_dim[l] > 512))
        return fail(DSDF_E_INVALID, "gemm_split needs every layer width <= 512 (layer %d: %d -> %d)", l, n->in_dim[l], n->out_dim[l]);
  }
  if (n->ln_param_mask) {
    if (n->weight_norm_mask) return fail(DSDF_E_INVALID, "LayerNorm (ln_param_mask) and weight norm exclude each other");
    if (n->ln_param_mask >> n->n_layers) return fail(DSDF_E_INVALID, "ln_param_mask names a layer >= n_layers");
    for (int l = 0; l < n->n_layers; ++l)
      if (((n->ln_param_mask >> l) & 1) && n->out_dim[l] > 2048) return fail(DSDF_E_INVALID, "LayerNorm width %d > 2048", n->out_dim[l]);
  }
  if (n->in_dim[n->n_layers - 1] % 4 != 0) return fail(DSDF_E_INVALID, "last hidden width must be a multiple of 4");
  if (!(n->dropout_p >= 0.f && n->dropout_p < 1.f)) return fail(DSDF_E_INVALID, "dropout_p must be in [0,1)");
  return 0;
}

struct Packed {
  int64_t w_off[DSDF_MAX_LAYERS], wt_off[DSDF_MAX_LAYERS];
  int ldw[DSDF_MAX_LAYERS], ldwt[DSDF_MAX_LAYERS];
  int64_t scale_off;   // per-row weight-norm scales of all layers
  // fragment-ordered copies for the fused kernels: Wf (n = out, k = in), WTf (n = in, k = out)
  int64_t wf_off[DSDF_MAX_LAYERS], wtf_off[DSDF_MAX_LAYERS];
  int64_t wfb_off[DSDF_MAX_LAYERS];   // bf16 fragment copy of W for the bf16 forward (fused_bf16x8.hpp); offset in floats
  int uf[DSDF_MAX_LAYERS], utf[DSDF_MAX_LAYERS];   // k-units of 16 per n-tile
  int64_t ws_off[DSDF_MAX_LAYERS], wts_off[DSDF_MAX_LAYERS];       // gemm_split: 3 bf16 planes of W / W^T in fragment order (offsets in floats)
  int64_t ws_plane[DSDF_MAX_LAYERS], wts_plane[DSDF_MAX_LAYERS];   //   bf16 elements per plane
  int64_t total;
};
Packed packed_layout(const DsdfNet* n) {
  Packed p;
  int64_t o = 0;
  for (int l = 0; l < n->n_layers; ++l) {
    p.ldw[l] = (int)rup(n->in_dim[l], 32);
    p.ldwt[l] = (int)rup(n->out_dim[l], 32);
    p.w_off[l] = o;  o += rup((int64_t)n->out_dim[l] * p.ldw[l], 64);
    p.wt_off[l] = o; o += rup((int64_t)n->in_dim[l] * p.ldwt[l], 64);
  }
  p.scale_off = o;
  for (int l = 0; l < n->n_layers; ++l) o += n->out_dim[l];
  o = rup(o, 64);
  for (int l = 0; l < n->n_layers; ++l) {
    const int64_t ntw = rup((n->out_dim[l] + 31) / 32, 4), ntt = rup((n->in_dim[l] + 31) / 32, 4);
    p.uf[l] = 2 * ((n->in_dim[l] + 31) / 32);
    p.utf[l] = 2 * ((n->out_dim[l] + 31) / 32);
    p.wf_off[l] = o;  o += ntw * p.uf[l] * 512;
    p.wtf_off[l] = o; o += ntt * p.utf[l] * 512;
    p.wfb_off[l] = o; o += n->fwd_bf16 ? ntw * 32 * 256 : 0;   // 32 phase-major k-unit slots of 1 KiB per n-tile
    p.ws_plane[l] = ntw * p.uf[l] * 512; p.wts_plane[l] = ntt * p.utf[l] * 512;     // (1 KiB = 512 bf16 per tile and k-unit)
  }
  o = rup(o, 64);
  for (int l = 0; l < n->n_layers; ++l) {   // gemm_split: the bf16 planes come LAST, so everything in front keeps its place
    p.ws_off[l] = o;  o += n->gemm_split ? 3 * p.ws_plane[l] / 2 : 0;
    p.wts_off[l] = o; o += n->gemm_split ? 3 * p.wts_plane[l] / 2 : 0;
  }
  p.total = rup(o, 64);
  return p;
}

void param_layout(const DsdfNet* n, DsdfParamLayout* L) {
  int64_t o = 0;
  for (int l = 0; l < DSDF_MAX_LAYERS; ++l) L->bias_off[l] = L->g_off[l] = L->v_off[l] = L->ln_w_off[l] = L->ln_b_off[l] = -1;
  for (int l = 0; l < n->n_layers; ++l) {
    const int64_t out = n->out_dim[l], in = n->in_dim[l];
    if ((n->weight_norm_mask >> l) & 1) {
      L->bias_off[l] = o; o += out;
      L->g_off[l] = o;    o += out;
      L->v_off[l] = o;    o += out * in;
    } else {
      L->v_off[l] = o;    o += out * in;
      L->bias_off[l] = o; o += out;
    }
    if ((n->ln_param_mask >> l) & 1) {   // bn{l}.weight, bn{l}.bias follow lin{l}'s parameters (module registration order)
      L->ln_w_off[l] = o; o += out;
      L->ln_b_off[l] = o; o += out;
    }
  }
  L->total = o;
}

// ---- dW work schedule (dwstream.hpp): (layer, K-split, 128x128 tile) items, ~one per wave of the chip ------------
struct DwSched {
  int tiles_m[DSDF_MAX_LAYERS], tiles_n[DSDF_MAX_LAYERS], last_nj[DSDF_MAX_LAYERS], nfull_n[DSDF_MAX_LAYERS],
      nsplit[DSDF_MAX_LAYERS], kchunk[DSDF_MAX_LAYERS], full0[DSDF_MAX_LAYERS], narrow0[DSDF_MAX_LAYERS];
  long long slab[DSDF_MAX_LAYERS];
  int n_full, n_narrow;
};
// waves of the CURRENT device (4 per CU).  The CU count is an immutable property of a device, cached per device ordinal
// (relaxed atomics: every writer stores the same value), so processes / threads driving different devices each get
// their own device's schedule -- no first-device-wins global.
int chip_waves() {
  constexpr int MAXDEV = 64;
  static std::atomic<int> cache[MAXDEV];
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 4 * 256;   // MI355X
  if (dev < MAXDEV) {
    const int w = cache[dev].load(std::memory_order_relaxed);
    if (w > 0) return w;
  }
  int waves = 4 * 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) waves = 4 * cus;
  if (dev < MAXDEV) cache[dev].store(waves, std::memory_order_relaxed);
  return waves;
}
int skip_layer(const DsdfNet* n) {
  for (int l = 1; l < n->n_layers - 1; ++l)
    if ((n->skip_mask >> l) & 1) return l;
  return -1;
}
// latent_in names the OUTPUT layer (valid in the reference: deep_sdf_decoder.py:88-89 runs for every layer incl. the last Linear): its
// input is [a | x0].  No segment mode, no dsdf_decode_latent for such a net; the heads route the x0 columns' gradient (kernels.hpp LastArgs).
bool last_layer_skip(const DsdfNet* n) { return ((n->skip_mask >> (n->n_layers - 1)) & 1) != 0; }
// columns of layer l's input that the dW GEMM contracts over the points: all of them, or -- segment mode -- only the
// previous layer's activations (the x0 columns of layer 0 / the skip layer are hoisted: finalize_row, kernels.hpp)
int dw_cols(const DsdfNet* n, int l, bool segmode) {
  if (!segmode) return n->in_dim[l];
  if (l == 0) return 0;
  return l == skip_layer(n) ? n->out_dim[l - 1] : n->in_dim[l];
}
// Layers [l0, l1) only (the others get no items): the two-phase backward of a data-parallel step (DsdfLossCfg.dw_phase) schedules
// each half of the layers so that it fills the chip by itself.
// reserve: waves the K-split leaves free on purpose -- phase 1 of a phased backward in segment mode keeps 16 workgroups for the riding
// post-backward roles (without them the roles are a launch of their own: +21 us per step)
DwSched dw_schedule(const DsdfNet* n, int64_t N, const int* ld_in, bool segmode, int l0 = 0, int l1 = DSDF_MAX_LAYERS, int reserve = 0) {
  DwSched S;
  memset(&S, 0, sizeof(S));
  const int nh = n->n_layers - 1;
  int Tfull = 0, Tnarrow = 0;
  for (int l = 0; l < nh; ++l) {
    const int nc = (l >= l0 && l < l1) ? dw_cols(n, l, segmode) : 0;
    S.slab[l] = rup((int64_t)n->out_dim[l] * ld_in[l], 64);
    if (nc == 0) { S.last_nj[l] = 4; continue; }   // no items
    S.tiles_m[l] = (n->out_dim[l] + 127) / 128;
    S.tiles_n[l] = (nc + 127) / 128;
    S.last_nj[l] = ((nc - (S.tiles_n[l] - 1) * 128) + 31) / 32;
    S.nfull_n[l] = S.last_nj[l] == 4 ? S.tiles_n[l] : S.tiles_n[l] - 1;
    Tfull += S.tiles_m[l] * S.nfull_n[l];
    if (S.last_nj[l] != 4) Tnarrow += S.tiles_m[l];
  }
  // one K-split count for every layer: the largest that still gives every wave of the chip at most one full item.  A net WITHOUT
  // full-width tiles (every layer narrower than 128: the reference's shipped 4 x 64 / 4 x 32 specs) is split by its narrow items
  // instead -- round 3 left such nets at ONE split, i.e. one wave contracting all the points of a layer.
  const int Tsplit = Tfull > 0 ? Tfull : Tnarrow;
  const int waves = chip_waves() - reserve > 0 ? chip_waves() - reserve : chip_waves();
  int ns = Tsplit > 0 && waves / Tsplit > 0 ? waves / Tsplit : 1;
  const int maxsplit = N / 64 > 0 ? (int)(N / 64) : 1;
  if (ns > maxsplit) ns = maxsplit;
  int kchunk = (int)rup((N + ns - 1) / ns, 2);
  if (kchunk < 2) kchunk = 2;   // N == 0 (size queries for an empty batch)
  ns = (int)((N + kchunk - 1) / kchunk);
  if (ns < 1) ns = 1;
  int nf = 0, nn = 0;
  for (int l = 0; l < nh; ++l) {
    S.nsplit[l] = S.tiles_m[l] > 0 ? ns : 0; S.kchunk[l] = kchunk;
    S.full0[l] = nf;   nf += ns * S.tiles_m[l] * S.nfull_n[l];
    S.narrow0[l] = nn; nn += S.last_nj[l] == 4 ? 0 : ns * S.tiles_m[l];
  }
  S.n_full = nf; S.n_narrow = nn;
  return S;
}

// K-bucket gradient exchange (data parallel): the decoder's layers are cut into K contiguous groups, handed out LAST layer
// first (the order the backward finishes them in): bucket b = layers [cut[b + 1], cut[b]), cut[0] = n_layers, cut[K] = 0.
// K = 2 on the 8 x 512 net: layers [4, 8] (1.05 M parameters) then [0, 4) (0.79 M).  A net with fewer layers than buckets
// leaves the trailing buckets empty (cut repeats 0).
void dw_bucket_cuts(const DsdfNet* n, int K, int* cut) {
  for (int b = 0; b <= K; ++b) cut[b] = (int)((int64_t)n->n_layers * (K - b) / K);
}

// ---- workspace plan -----------------------------------------------------------------------------
// Debug-only view of the planners (dsdf_debug_ws_redzone / dsdf_debug_ws_regions, include/dsdf.h).  Every take() of a planner
// is followed by g_redzone unused bytes (0 by default: the layout is then exactly the one without this mechanism), and a planner
// that is handed a WsTable writes one {name, offset, exact bytes} row per take().  Every entry point that launches on a
// workspace hands its planner the thread's t_last_plan, so a test can read the layout a launch actually used and compare
// every byte outside the regions with what it put there.  Recording is a few stores per take(): no string is formatted
// before the table is read.
std::atomic<size_t> g_redzone{0};
struct WsRow { const char* name; int idx; size_t off, bytes; };
struct WsTable {
  int n, dropped;
  size_t total;
  WsRow row[DSDF_WS_MAX_REGIONS];
  void reset() { n = 0; dropped = 0; total = 0; }
  void add(const char* name, int idx, size_t off, size_t bytes) {
    if (n < DSDF_WS_MAX_REGIONS) row[n++] = WsRow{name, idx, off, bytes};
    else ++dropped;
  }
};
thread_local WsTable t_last_plan;

// What every planner carves its regions with.  align: 256, or 1 where regions were never padded (mesh SDF, nearest neighbour, and
// the two test entries dsdf_gemm_tn / dsdf_grad_norm).
struct WsCarver {
  size_t o = 0, guard, align;
  WsTable* rec;
  explicit WsCarver(WsTable* r, size_t al = 256) : guard(g_redzone.load(std::memory_order_relaxed)), align(al), rec(r) {
    if (rec) rec->reset();
  }
  size_t take(const char* name, int idx, size_t bytes) {
    const size_t r = o;
    o += (size_t)rup((int64_t)bytes, (int64_t)align) + guard;
    if (rec) rec->add(name, idx, r, bytes);
    return r;
  }
  size_t finish(size_t total) {   // total: o, or what the planner reports instead (decode_latent_plan)
    if (rec) rec->total = total;
    return total;
  }
};

struct Plan {
  int nl, W0, N, R;
  int ld_in[DSDF_MAX_LAYERS];
  size_t in_off[DSDF_MAX_LAYERS];
  int ld_dp, ldz, ldcs, ld_part, last_blocks, nsplit, kchunk, mt;
  long long slab;
  size_t u_off, y_off, dp_off[2], dzA_off, dzB_off, slab_off, colsum_off, part_off, part2_off, partdb_off,
      partloss_off, segpart_off, segnorm_off, gnorm_off, dxz_off[2], lnpg_off, lnpb_off, total;
  size_t lnx_off[DSDF_MAX_LAYERS], lnr_off[DSDF_MAX_LAYERS];   // LayerNorm: xhat [N][ld_in[l+1]] (the Linear's output in place), rstd [N]
  // fused backward: per hidden layer l a global dP_l buffer, the forward's mask bits and per-workgroup column sums
  size_t dpl_off[DSDF_MAX_LAYERS], mask_off[DSDF_MAX_LAYERS], cs_off[DSDF_MAX_LAYERS], dwslab_off[DSDF_MAX_LAYERS];
  int nwg, frows;    // workgroups of the fused kernels and their rows (64; 32 for batches that would leave CUs idle: pick_path)
  DwSched dw;
  DwSched dwph[DSDF_MAX_BUCKETS];   // phased backward: the schedule of bucket b's layers [dw_cut[b + 1], dw_cut[b])
  int dw_nb, dw_cut[DSDF_MAX_BUCKETS + 1];   // dw_bucket_cuts
  // segment mode: U[R][2][ldu] of the hoisted layers, per-workgroup xyz sums [nwg][4][ldcs] for each of them
  int segmode, ldu, ldh;
  long long hstride;
  size_t hoistU_off, xsum_off[2], hs_off, zr_off;   // hs: [2][maxout][ldh] x0 columns of the hoisted layers' weight gradients
};

// nb: the bucket count the workspace is laid out for (DsdfLossCfg.dw_buckets; every call of one step passes the same one).
// 2 also serves the un-phased step, so dsdf_workspace_bytes' answer covers K <= 2.
// rec: the table that receives one row per take() (launching entry points: &t_last_plan; size queries: none).
Plan make_plan(const DsdfNet* n, int64_t N, int64_t R, bool inference, bool segmode = false, int nb = 2, int frows = FROWS,
               WsTable* rec = nullptr) {
  Plan P;
  memset(&P, 0, sizeof(P));
  P.frows = frows;
  P.nl = n->n_layers; P.W0 = n->latent_size + n->geom_dim; P.N = (int)N; P.R = (int)R;
  WsCarver c(rec);
  int maxw = 4;
  for (int l = 0; l < P.nl; ++l) {
    P.ld_in[l] = (int)rup(n->in_dim[l], 4);
    if (P.ld_in[l] > maxw) maxw = P.ld_in[l];
  }
  if (inference) {
    size_t pp[2] = {c.take("pp", 0, (size_t)N * maxw * 4), c.take("pp", 1, (size_t)N * maxw * 4)};
    for (int l = 0; l < P.nl; ++l) {
      // (xyz_in_all: every layer input carries xyz columns the gather pre-fills, so none of them can share a ping-pong buffer)
      if (l == 0 || ((n->skip_mask >> l) & 1) || n->xyz_in_all) P.in_off[l] = c.take("in", l, (size_t)N * P.ld_in[l] * 4);
      else P.in_off[l] = pp[l & 1];
    }
    if (n->ln_param_mask) {   // one scratch row block for the Linear's output before LayerNorm (nothing is kept in inference)
      const size_t t = c.take("lnx", -1, (size_t)N * maxw * 4);
      for (int l = 0; l < P.nl; ++l) P.lnx_off[l] = t;
    }
    P.total = c.finish(c.o);
    return P;
  }
  for (int l = 0; l < P.nl; ++l) P.in_off[l] = c.take("in", l, (size_t)N * P.ld_in[l] * 4 + 4096);   // + slack: edge tiles of dw_stream over-read
  P.u_off = c.take("u", -1, (size_t)N * 4);
  P.y_off = c.take("y", -1, (size_t)N * 4);
  P.ld_dp = maxw;
  P.dp_off[0] = c.take("dp", 0, (size_t)N * maxw * 4);
  P.dp_off[1] = c.take("dp", 1, (size_t)N * maxw * 4);
  P.ldz = (int)rup(P.W0, 4);
  P.dzA_off = c.take("dzA", -1, (size_t)N * P.ldz * 4);
  P.dzB_off = c.take("dzB", -1, (size_t)N * P.ldz * 4);
  for (int t = 0; t < 2; ++t) P.dxz_off[t] = n->xyz_in_all ? c.take("dxz", t, (size_t)N * 4 * 4) : 0;   // [N][4]: one layer's d/d(xyz), running sum
  for (int l = 0; l + 1 < P.nl; ++l)
    if ((n->ln_param_mask >> l) & 1) { P.lnx_off[l] = c.take("lnx", l, (size_t)N * P.ld_in[l + 1] * 4); P.lnr_off[l] = c.take("lnr", l, (size_t)N * 4); }
  // split-K of the dW GEMMs: chunks of >= 256 points, at most NSPLIT_MAX slabs
  int ns = (int)((N + 255) / 256);
  if (ns > NSPLIT_MAX) ns = NSPLIT_MAX;
  if (ns < 1) ns = 1;
  P.kchunk = (int)rup((N + ns - 1) / ns, BK);
  if (P.kchunk < BK) P.kchunk = BK;   // N == 0 (size query for an empty batch)
  P.nsplit = (int)((N + P.kchunk - 1) / P.kchunk);
  if (P.nsplit < 1) P.nsplit = 1;
  int64_t maxslab = 0;
  int maxout = 1;
  for (int l = 0; l < P.nl - 1; ++l) {
    const int64_t s = (int64_t)n->out_dim[l] * P.ld_in[l];
    if (s > maxslab) maxslab = s;
    if (n->out_dim[l] > maxout) maxout = n->out_dim[l];
  }
  P.slab = rup(maxslab, 64);
  P.slab_off = c.take("slab", -1, (size_t)P.nsplit * P.slab * 4);
  P.mt = (int)((N + BM - 1) / BM);
  P.ldcs = (int)rup(maxout, 4);
  P.colsum_off = c.take("colsum", -1, (size_t)P.mt * P.ldcs * 4);
  if (n->ln_param_mask) { P.lnpg_off = c.take("lnpg", -1, (size_t)LN_BLOCKS * P.ldcs * 4); P.lnpb_off = c.take("lnpb", -1, (size_t)LN_BLOCKS * P.ldcs * 4); }
  P.last_blocks = (int)((N + 15) / 16);
  if (P.last_blocks > LAST_BLOCKS_MAX) P.last_blocks = LAST_BLOCKS_MAX;
  if (P.last_blocks < 1) P.last_blocks = 1;
  P.ld_part = 2 * P.ld_in[P.nl - 1];  // [dW_last | colsum_prev]
  // one row of head partials per block of last_layer_kernel (<= LAST_BLOCKS_MAX) OR per workgroup of the fused backward (N / 64,
  // unbounded): sized for the larger.  (Rounds 1-3 sized them by last_blocks alone: batches of more than 65536 points -- the shipped
  // 10 x 16000 -- let the fused head write its partials past these buffers, into part2 / partdb / partloss and the dP_0 buffer.)
  const size_t part_rows = (size_t)std::max<int64_t>(P.last_blocks, (N + frows - 1) / frows);
  P.part_off = c.take("part", -1, part_rows * P.ld_part * 4);
  P.part2_off = c.take("part2", -1, (size_t)LAST_GROUPS * P.ld_part * 4);
  P.partdb_off = c.take("partdb", -1, part_rows * 4);
  P.partloss_off = c.take("partloss", -1, part_rows * 4);
  P.segpart_off = c.take("segpart", -1, (size_t)LAT_SLICES_MAX * (R > 0 ? R : 1) * (n->latent_size > 0 ? n->latent_size : 1) * 4);   // (up to 8 partial copies)
  P.segnorm_off = c.take("segnorm", -1, (size_t)(R > 0 ? R : 1) * 4);
  P.gnorm_off = c.take("gnorm", -1, 1024 * 4);
  P.nwg = (int)((N + frows - 1) / frows);
  for (int l = 0; l < P.nl - 1; ++l) {
    P.dpl_off[l] = c.take("dpl", l, (size_t)N * maxw * 4 + 4096);
    P.mask_off[l] = c.take("mask", l, (size_t)P.nwg * 256 * 16);
    P.cs_off[l] = c.take("cs", l, (size_t)P.nwg * P.ldcs * 4);
  }
  P.dw = dw_schedule(n, N, P.ld_in, segmode);
  P.dw_nb = nb < 2 ? 2 : (nb > DSDF_MAX_BUCKETS ? DSDF_MAX_BUCKETS : nb);
  dw_bucket_cuts(n, P.dw_nb, P.dw_cut);
  for (int t = 0; t < P.dw_nb; ++t)
    // (two buckets only: the riding roles take ~180 us, a bucket's launch must be at least that long or they become its tail --
    // measured: K = 2 1.3100 -> 1.3032 ms/step with the reserve, K = 4 1.3776 -> 1.4116)
    P.dwph[t] = dw_schedule(n, N, P.ld_in, segmode, P.dw_cut[t + 1], P.dw_cut[t],
                            t == 0 && P.dw_nb == 2 && segmode && P.nwg <= chip_waves() / 4 ? 64 : 0);
  for (int l = 0; l < P.nl - 1; ++l) {   // slabs sized for whichever schedule splits K finest: the layout does not depend on the phase
    int ns = P.dw.nsplit[l];
    for (int t = 0; t < P.dw_nb; ++t)
      if (P.dwph[t].nsplit[l] > ns) ns = P.dwph[t].nsplit[l];
    P.dwslab_off[l] = c.take("dwslab", l, (size_t)ns * P.dw.slab[l] * 4);
  }
  P.segmode = segmode ? 1 : 0;
  if (segmode) {
    P.ldu = P.ldcs;
    P.hoistU_off = c.take("hoistU", -1, (size_t)(R > 0 ? R : 1) * 2 * P.ldu * 4);
    for (int t = 0; t < 2; ++t) P.xsum_off[t] = c.take("xsum", t, (size_t)P.nwg * 4 * P.ldcs * 4);
    P.ldh = (int)rup(n->latent_size + n->geom_dim, 4);
    P.hstride = (long long)P.ldcs * P.ldh;
    P.hs_off = c.take("hs", -1, (size_t)2 * P.hstride * 4);
    P.zr_off = c.take("zr", -1, (size_t)(R > 0 ? R : 1) * (n->latent_size > 0 ? n->latent_size : 1) * 4);   // renormed latent row of every segment
  }
  P.total = c.finish(c.o);
  return P;
}

// ---- launch helpers -------------------------------------------------------------------------------
template <int EPI>
int launch_nt(const NtArgs& a, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0) return 0;
  if (a.K <= 0) return fail(DSDF_E_INVALID, "gemm_nt: K must be positive");
  if ((a.lda & 3) || (a.ldb & 3) || !aligned16(a.A) || !aligned16(a.B))
    return fail(DSDF_E_INVALID, "gemm_nt: operands must be 16-byte aligned with ld %% 4 == 0");
  if (a.lda < rup(a.K, 4) || a.ldb < rup(a.K, 4)) return fail(DSDF_E_INVALID, "gemm_nt: ld smaller than K rounded up to 4");
  const int grid = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  ProfScope ps(DSDF_PROF_GEMM_NT, 2.0 * a.M * a.N * a.K, st);
  hipLaunchKernelGGL(gemm_nt_kernel<EPI>, dim3(grid), dim3(256), 0, st, a);
  LAUNCH_OK("gemm_nt_kernel");
  return 0;
}

int launch_tn(const TnArgs& a, int nsplit, hipStream_t st) {
  if (a.M <= 0 || a.N <= 0 || nsplit <= 0) return 0;
  if ((a.lda & 3) || (a.ldb & 3) || !aligned16(a.A) || !aligned16(a.B))
    return fail(DSDF_E_INVALID, "gemm_tn: operands must be 16-byte aligned with ld %% 4 == 0");
  if (a.lda < rup(a.M, 4) || a.ldb < rup(a.N, 4)) return fail(DSDF_E_INVALID, "gemm_tn: ld smaller than the tile width");
  if (a.kchunk % BK) return fail(DSDF_E_INVALID, "gemm_tn: kchunk must be a multiple of %d", BK);
  const int grid = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN) * nsplit;
  ProfScope ps(DSDF_PROF_GEMM_TN, 2.0 * a.M * a.N * a.K, st);
  hipLaunchKernelGGL(gemm_tn_kernel, dim3(grid), dim3(256), 0, st, a);
  LAUNCH_OK("gemm_tn_kernel");
  return 0;
}

template <int MODE>
int launch_last(const LastArgs& a, int blocks, hipStream_t st) {
  if (a.n <= 0) return 0;
  const int in = a.in;
  ProfScope ps(DSDF_PROF_LAST, (MODE == LAST_FWD ? 2.0 : 6.0) * a.n * a.in, st);
  if (in <= 256) hipLaunchKernelGGL((last_layer_kernel<MODE, 1>), dim3(blocks), dim3(256), 0, st, a);
  else if (in <= 512) hipLaunchKernelGGL((last_layer_kernel<MODE, 2>), dim3(blocks), dim3(256), 0, st, a);
  else if (in <= 1024) hipLaunchKernelGGL((last_layer_kernel<MODE, 4>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((last_layer_kernel<MODE, 8>), dim3(blocks), dim3(256), 0, st, a);
  LAUNCH_OK("last_layer_kernel");
  return 0;
}

// Adam constants of one parameter group (torch/optim/adam.py single-tensor form; bias corrections in double on the host)
AdamRide adam_ride(float* p, const float* g, float* m, float* v, int64_t n, float lr, const DsdfAdamCfg* c) {
  AdamRide a;
  memset(&a, 0, sizeof(a));
  const double bc1 = 1.0 - pow((double)c->beta1, (double)c->step), bc2 = 1.0 - pow((double)c->beta2, (double)c->step);
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n;
  a.blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  a.omb1 = 1.0f - c->beta1; a.b2 = c->beta2; a.omb2 = 1.0f - c->beta2;
  a.step_size = (float)((double)lr / bc1); a.bc2_sqrt = (float)sqrt(bc2); a.eps = c->eps;
  return a;
}

// ride != nullptr: a dense Adam update (the latent table) done by extra blocks of the wn_tiles launch
int materialize(const DsdfNet* net, const float* params, float* packed, hipStream_t st, bool scales_ready = false,
                const AdamRide* ride = nullptr) {
  DsdfParamLayout L;
  param_layout(net, &L);
  const Packed pk = packed_layout(net);
  WnAll a;
  memset(&a, 0, sizeof(a));
  a.nl = net->n_layers;
  a.scale = packed + pk.scale_off;
  int rows = 0, tiles = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    WnLayer& y = a.ly[l];
    y.v = params + L.v_off[l];
    y.g = L.g_off[l] >= 0 ? params + L.g_off[l] : nullptr;
    y.W = packed + pk.w_off[l];
    y.WT = (l == net->n_layers - 1) ? nullptr : packed + pk.wt_off[l];
    y.out = net->out_dim[l]; y.in = net->in_dim[l]; y.ldw = pk.ldw[l]; y.ldwt = pk.ldwt[l];
    y.row0 = rows; y.tile0 = tiles; y.tcols = (y.in + 31) / 32;
    const bool last = l == net->n_layers - 1;
    y.Wf = last ? nullptr : packed + pk.wf_off[l];
    y.WTf = last ? nullptr : packed + pk.wtf_off[l];
    y.Wfb = (last || !net->fwd_bf16) ? nullptr : reinterpret_cast<__bf16*>(packed + pk.wfb_off[l]);
    y.Uf = pk.uf[l]; y.UTf = pk.utf[l];
    const bool sp = net->gemm_split && !last;
    y.Ws = sp ? reinterpret_cast<__bf16*>(packed + pk.ws_off[l]) : nullptr;
    y.WTs = sp ? reinterpret_cast<__bf16*>(packed + pk.wts_off[l]) : nullptr;
    y.ws_plane = pk.ws_plane[l]; y.wts_plane = pk.wts_plane[l];
    rows += y.out;
    tiles += ((y.out + 31) / 32) * y.tcols;
  }
  a.total_rows = rows; a.total_tiles = tiles;
  if (!scales_ready) {   // dsdf_train_step's fused finalize+Adam already wrote the new row scales
    hipLaunchKernelGGL(wn_scale_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a);
    LAUNCH_OK("wn_scale_kernel");
  }
  if (ride != nullptr) a.adam = *ride;
  hipLaunchKernelGGL(wn_tiles_kernel, dim3(tiles + a.adam.blocks), dim3(256), 0, st, a);
  LAUNCH_OK("wn_tiles_kernel");
  return 0;
}

constexpr float LATENT_DROPOUT_P = 0.2f;          // nn.Dropout(0.2), deep_sdf_decoder.py:36
constexpr int LATENT_DROPOUT_KEY = DSDF_MAX_LAYERS - 1;   // slot of dropout_key[] (no hidden layer can have this index)
inline uint32_t latent_drop_thr() { return (uint32_t)lround((double)LATENT_DROPOUT_P * 65536.0); }
inline bool net_variant(const DsdfNet* n) { return n->latent_dropout || n->xyz_in_all || n->ln_param_mask != 0; }
inline bool ln_applied(const DsdfNet* n, int l) { return ((n->ln_param_mask >> l) & 1) && l < n->n_layers - 1; }   // hidden layers only

// ---- the kernel path of one call --------------------------------------------------------------------
// A/B and test switches.  Read ONCE per call, by open_call (the tests flip them inside one process); nothing below an entry
// point reads the environment (lab builds and the per-process DSDF_NO_RIDE of plan_roles excepted).
struct Switches {
  bool no_fused, no_narrow, frows64, no_w32, no_w32x2, no_merge;
  static Switches read() {
    auto is1 = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
    const char* fr = getenv("DSDF_FROWS");
    Switches s;
    s.no_fused = is1("DSDF_NO_FUSED");             // the layer-by-layer launches instead of the fused kernels
    s.no_narrow = is1("DSDF_NO_NARROW");           // narrow nets on the full-size kernels
    s.frows64 = fr && !strcmp(fr, "64");           // no 32-row workgroups
    s.no_w32 = getenv("DSDF_NO_W32") != nullptr;   // no wave-private kernels (w32x2: the 64-wide one only)
    s.no_w32x2 = getenv("DSDF_NO_W32X2") != nullptr;
    s.no_merge = getenv("DSDF_NO_MERGE") != nullptr;   // training: forward and backward as two launches
#ifdef DSDF_LAB
    if (getenv("DSDF_LAB_DBG")) s.no_merge = true;     // per-layer stamps are dumped after a forward launch of its own
#endif
    return s;
  }
};

enum Family { FAM_LAYERED, FAM_FP32, FAM_SPLIT, FAM_BF16, FAM_BF16_SPLIT, FAM_H32, FAM_N128, FAM_W32, FAM_W32X2, FAM_COUNT };
enum Entry { ENTRY_TRAIN, ENTRY_MODULE_FWD, ENTRY_MODULE_BWD, ENTRY_INFER };
struct Path {
  Family family;
  int frows;     // rows per workgroup of the fused kernels: what make_plan lays the per-workgroup regions out for
  bool fused;    // family != FAM_LAYERED
  bool merged;   // training: forward + backward of the same points go out as one launch
};

// One row per family: the kernel of every role (nullptr: the family has none) and the block sizes.
using FwdKernel = void (*)(FusedFwdArgs);
using BwdKernel = void (*)(FusedBwdArgs);
using FwdBwdKernel = void (*)(FusedFwdArgs, FusedBwdArgs);
using DwKernel = void (*)(DwArgs, PostBwdArgs, int, int);
struct FamilyKernels {
  FwdKernel fwd; int fwd_block;   // forward without activation copies (inference)
  FwdKernel fwd_act;              // forward with activation copies (module path, un-merged training)
  BwdKernel bwd;                  // separate backward: 64-row workgroups only
  FwdBwdKernel fwd_bwd;           // merged forward + backward
  DwKernel dw;
  int block;                      // every role but fwd
};
const FamilyKernels KERNELS[FAM_COUNT] = {
    /* FAM_LAYERED    */ {nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0},
    /* FAM_FP32       */ {fused_forward_kernel, 256, fused_forward_kernel, fused_backward_kernel, fused_fwd_bwd_kernel, dw_stream_kernel, 256},
    /* FAM_SPLIT      */ {fused_forward_split_kernel, 256, fused_forward_split_kernel, fused_backward_split_kernel, fused_fwd_bwd_split_kernel,
                          dw_stream_split_kernel, 256},
    // config 5: the inference form has 8 staggered waves and transposed accumulators (fused_bf16x8.hpp); the backward is fp32
    /* FAM_BF16       */ {fused_forward_bf16x8_kernel, F8_THREADS, fused_forward_bf16_kernel, fused_backward_kernel, fused_fwd_bf16_bwd_kernel,
                          dw_stream_kernel, 256},
    /* FAM_BF16_SPLIT */ {fused_forward_bf16x8_kernel, F8_THREADS, fused_forward_bf16_kernel, fused_backward_split_kernel,
                          fused_fwd_bf16_bwd_split_kernel, dw_stream_split_kernel, 256},
    /* FAM_H32        */ {fused_forward_h32_kernel, 256, fused_forward_h32_kernel, nullptr, fused_fwd_bwd_h32_kernel, dw_stream_kernel, 256},
    /* FAM_N128       */ {fused_forward_n128_kernel, 256, fused_forward_n128_kernel, fused_backward_kernel, fused_fwd_bwd_n128_kernel,
                          dw_stream_kernel, 256},
    // wave-private: one wave per workgroup, merged training launch only
    /* FAM_W32        */ {nullptr, 0, nullptr, nullptr, fused_fwd_bwd_w32_kernel, dw_stream_kernel, 64},
    /* FAM_W32X2      */ {nullptr, 0, nullptr, nullptr, fused_fwd_bwd_w32x2_kernel, dw_stream_kernel, 64},
};

bool fused_eligible(const DsdfNet* net) {
  if (net_variant(net)) return false;   // latent_dropout / xyz_in_all live on the layer-by-layer kernels only
  if (net->in_dim[0] > FMAXW) return false;
  for (int l = 0; l < net->n_layers - 1; ++l)
    if (net->in_dim[l] > FMAXW || net->out_dim[l] > FMAXW) return false;
  return net->in_dim[net->n_layers - 1] <= FMAXW;
}

// THE decision which kernels run a call of `entry` on n points (n <= 0: the family whatever the batch).  Precedence, first match:
//   not fused (DSDF_NO_FUSED, or a net the fused kernels do not cover)        -> layered
//   bf16 / gemm_split nets                                                    -> their own family, 64 rows
//   module entry points, un-merged training, DSDF_FROWS=64                    -> n128 for narrow nets, else fp32; 64 rows
//   merged training, narrow net of at most 32- / 64-wide layers               -> w32 / w32x2 (wave-private: 32 points per one-wave
//                                                                                workgroup) at EVERY batch size
//   batches of at most 32 points per CU (64-row workgroups would leave at least half of the chip idle: BASELINE config 4,
//   one shape x 8000 points) -- inference and merged training                 -> h32, 32 rows, for narrow nets too
//   otherwise                                                                 -> n128 for narrow nets, else fp32; 64 rows
// Narrow: every layer input and hidden width <= 128 (the n128 variants run two workgroups per CU, fused.hpp); fp32 MFMA only.
Path pick_path(const DsdfNet* net, int64_t n, Entry entry, const Switches& sw) {
  Path p{FAM_LAYERED, FROWS, false, false};
  if (sw.no_fused || !fused_eligible(net)) return p;
  p.fused = true;
  p.merged = entry == ENTRY_TRAIN && !sw.no_merge;
  if (net->fwd_bf16 || net->gemm_split) {
    p.family = !net->fwd_bf16 ? FAM_SPLIT : (net->gemm_split ? FAM_BF16_SPLIT : FAM_BF16);
    return p;
  }
  int wmax = 0;
  for (int l = 0; l < net->n_layers; ++l) {
    wmax = std::max(wmax, net->in_dim[l]);
    if (l < net->n_layers - 1) wmax = std::max(wmax, net->out_dim[l]);
  }
  const bool narrow = !sw.no_narrow && wmax <= 128;
  p.family = narrow ? FAM_N128 : FAM_FP32;
  const bool rows32 = entry == ENTRY_INFER || p.merged;   // (the separate backward kernel and the module path's plan keep 64 rows)
  if (!rows32 || sw.frows64 || n <= 0) return p;
  if (p.merged && narrow && !sw.no_w32 && (wmax <= FWW || (wmax <= FWW2 && !sw.no_w32x2))) {
    p.family = wmax <= FWW ? FAM_W32 : FAM_W32X2;
    p.frows = 32;
  } else if (n <= 32ll * (chip_waves() / 4)) {
    p.family = FAM_H32;
    p.frows = 32;
  }
  return p;
}

// dropout of hidden layer `layer`'s output: the 16-bit keep threshold and the scale of what is kept
struct Drop { bool on; uint32_t thr; float scale; };
Drop drop_of(const DsdfNet* net, int layer, int training) {
  Drop d{training && ((net->dropout_mask >> layer) & 1) && net->dropout_p > 0.f, 0u, 1.0f};
  if (d.on) {
    d.thr = (uint32_t)std::min(lround((double)net->dropout_p * 65536.0), 65535l);
    d.scale = 1.0f / (1.0f - net->dropout_p);
  }
  return d;
}
float mask_scale_of(const DsdfNet* net, int layer, int training) { return drop_of(net, layer, training).scale; }

// The state of one call: everything the launch code below an entry point works on, filled ONCE, by open_call.  The helpers take it
// whole and add only what is their own.  No behaviour: fields, and the typed view of a workspace region.
struct Call {
  const DsdfNet* net;
  Switches sw;
  Path path;
  Plan P;
  DsdfParamLayout L;   // where each layer's parameters sit in params / grads
  Packed pk;           // ... and its materialized copies in packed
  void* ws;
  const float* packed;
  const float* params;
  int64_t n;
  hipStream_t st;
  int training;           // these three: zero behind open_call, the training / module entries set them
  const uint32_t* keys;   // dropout keys of the layers (+ LATENT_DROPOUT_KEY)
  uint32_t row_offset;    // of this call's first point in the dropout hash (data-parallel ranks)
  template <typename T>
  T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }
};

// x0 (+ skip copies, + the xyz columns of every layer of an xyz_in_all net) from either the latent table + segments or an
// explicit input; keys != nullptr && training: latent_dropout nets drop layer 0's latent columns on the way
int run_gather(const Call& c, const float* table, const DsdfBatch* b, const float* input, int64_t ld_in) {
  GatherArgs g;
  memset(&g, 0, sizeof(g));
  g.table = table; g.L = c.net->latent_size; g.G = c.net->geom_dim;
  if (b) { g.xyz = b->xyz; g.seg_scene = b->seg_scene; g.seg_offset = b->seg_offset; g.R = (int)b->n_segments; }
  g.input = input; g.ld_in = ld_in; g.n = (int)c.n;
  const int W0 = c.net->latent_size + c.net->geom_dim;
  const bool drop = c.net->latent_dropout && c.training && c.keys != nullptr && c.net->latent_size > 0;
  if (drop) { g.drop_key = c.keys[LATENT_DROPOUT_KEY]; g.drop_thr = latent_drop_thr(); g.drop_scale = 1.0f / (1.0f - LATENT_DROPOUT_P); g.row_offset = c.row_offset; }
  g.ndst = 0;
  g.dst[g.ndst++] = GatherDst{c.at<float>(c.P.in_off[0]), c.P.ld_in[0], 0, 0, W0, drop ? 1 : 0};
  for (int l = 1; l < c.net->n_layers; ++l) {
    if ((c.net->skip_mask >> l) & 1) g.dst[g.ndst++] = GatherDst{c.at<float>(c.P.in_off[l]), c.P.ld_in[l], c.net->out_dim[l - 1], 0, W0, 0};
    else if (c.net->xyz_in_all) g.dst[g.ndst++] = GatherDst{c.at<float>(c.P.in_off[l]), c.P.ld_in[l], c.net->out_dim[l - 1], c.net->latent_size, c.net->geom_dim, 0};
  }
  hipLaunchKernelGGL(gather_concat_kernel, dim3((unsigned)((c.n + 3) / 4)), dim3(256), 0, c.st, g);
  LAUNCH_OK("gather_concat_kernel");
  return 0;
}

#ifdef DSDF_LAB
// lab builds: device buffers of per-wave clock stamps.  One static LabStamps per launch site (allocated once, when the environment
// names a dump file); a LabScope around the launch zeroes it on the stream (sites that ask for it) and, when the scope ends,
// synchronises the device and writes the stamps to that file.
struct LabStamps { const char* env; size_t bytes; bool zero; unsigned long long* dev; };
struct LabScope {
  LabStamps& s;
  LabScope(LabStamps& site, hipStream_t st) : s(site) {
    if (!s.dev && getenv(s.env)) (void)hipMalloc(&s.dev, s.bytes);
    if (s.dev && s.zero) (void)hipMemsetAsync(s.dev, 0, s.bytes, st);
  }
  ~LabScope() {
    if (!s.dev || !getenv(s.env)) return;
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h(s.bytes / 8);
    (void)hipMemcpy(h.data(), s.dev, s.bytes, hipMemcpyDeviceToHost);
    FILE* f = fopen(getenv(s.env), "wb");
    if (f) { fwrite(h.data(), 1, s.bytes, f); fclose(f); }
  }
};
#endif

// all hidden layers + the last layer's forward in ONE launch (fused.hpp).  store_act: keep global copies of the
// activations (training / module path) or not (inference).
// Segment mode: U[s][t][:] = W_t[:, latent columns] latent_s for layer 0 (t = 0) and the skip layer (t = 1), and the
// descriptor the fused forward needs to start its accumulators from them.
// renorm != nullptr (training steps): the launch also does the max-norm renorm of the looked-up rows into zr (max_norm <= 0: a plain
// copy) and zeroes the dense latent gradient (nzero floats of dlat; 0: leaves it) -- no latent_renorm_kernel launch in segment mode
struct HoistRenorm { float max_norm; float* dlat; long long nzero; };
int run_hoist(const Call& c, const float* table, const DsdfBatch* b, FusedSeg* seg, const HoistRenorm* renorm = nullptr) {
  // (seg_hoist_kernel clamps its loads to column latent_size - 1: there must be one.  Both callers exclude the case before they
  // get here -- the segment-mode condition and decode_latent_ok -- so this is the guard of a third one)
  if (c.net->latent_size < 1 || c.net->latent_size > HOIST_MAXL)
    return fail(DSDF_E_INVALID, "segment mode needs 1 <= latent_size <= %d (got %d)", HOIST_MAXL, c.net->latent_size);
  const int ks = skip_layer(c.net);
  HoistArgs h;
  memset(&h, 0, sizeof(h));
  memset(seg, 0, sizeof(*seg));
  h.nh = ks > 0 ? 2 : 1;
  h.W[0] = c.packed + c.pk.w_off[0]; h.ldw[0] = c.pk.ldw[0]; h.c0[0] = 0; h.out[0] = c.net->out_dim[0];
  seg->h[0].layer = 0; seg->h[0].wx = h.W[0] + c.net->latent_size; seg->h[0].ldw = c.pk.ldw[0];
  seg->h[1].layer = -1;
  if (ks > 0) {
    h.W[1] = c.packed + c.pk.w_off[ks]; h.ldw[1] = c.pk.ldw[ks]; h.c0[1] = c.net->out_dim[ks - 1]; h.out[1] = c.net->out_dim[ks];
    seg->h[1].layer = ks; seg->h[1].wx = h.W[1] + h.c0[1] + c.net->latent_size; seg->h[1].ldw = c.pk.ldw[ks];
  }
  h.L = c.net->latent_size; h.seg_scene = b->seg_scene; h.table = table; h.R = (int)b->n_segments;
  h.U = c.at<float>(c.P.hoistU_off); h.ldu = c.P.ldu;
  h.bf16 = c.net->fwd_bf16 ? 1 : 0;
  if (renorm != nullptr) {
    h.max_norm = renorm->max_norm; h.zr = c.at<float>(c.P.zr_off);
    h.dlat = renorm->nzero > 0 ? renorm->dlat : nullptr; h.nzero = renorm->nzero;
  }
  const int rows = h.out[0] + (ks > 0 ? h.out[1] : 0);
  const dim3 hgrid((unsigned)((rows + 3) / 4), (unsigned)((h.R + HOIST_SC - 1) / HOIST_SC));
  switch ((h.L + 63) >> 6) {               // k-units of 64 latent columns per lane (HOIST_MAXL = 512)
    case 1: hipLaunchKernelGGL(seg_hoist_kernel<1>, hgrid, dim3(256), 0, c.st, h); break;
    case 2: hipLaunchKernelGGL(seg_hoist_kernel<2>, hgrid, dim3(256), 0, c.st, h); break;
    case 3: case 4: hipLaunchKernelGGL(seg_hoist_kernel<4>, hgrid, dim3(256), 0, c.st, h); break;
    default: hipLaunchKernelGGL(seg_hoist_kernel<8>, hgrid, dim3(256), 0, c.st, h); break;
  }
  LAUNCH_OK("seg_hoist_kernel");
  seg->wg_per_seg = (int)(b->seg_len / c.P.frows);
  seg->xyz = b->xyz; seg->G = c.net->geom_dim; seg->U = h.U; seg->ldu = h.ldu;
  return 0;
}

// seg != nullptr: segment mode (fused.hpp FusedSeg) -- x0 is not read at all, seg->h[] / seg->U come from run_hoist
int run_fused_forward(const Call& c, bool store_act, float* y_out, float* u_out, const FusedSeg* seg = nullptr,
                      FusedFwdArgs* defer = nullptr) {
  // defer != nullptr: fill *defer and launch nothing -- the caller hands it to run_backward_fused, which launches forward and
  // backward as ONE kernel (fused_fwd_bwd_kernel)
  const int last = c.net->n_layers - 1;
  FusedFwdArgs a;
  memset(&a, 0, sizeof(a));
  a.n_hidden = last; a.N = (int)c.n; a.W0 = c.net->in_dim[0];
  a.x0 = c.at<float>(c.P.in_off[0]); a.ldx0 = c.P.ld_in[0];
  a.row_offset = c.row_offset;
  for (int l = 0; l < last; ++l) {
    FusedLayer& y = a.ly[l];
    y.wf = c.net->fwd_bf16 ? c.packed + c.pk.wfb_off[l] : (c.net->gemm_split ? c.packed + c.pk.ws_off[l] : c.packed + c.pk.wf_off[l]);   // (bf16 copy / split planes)
    y.wplane = (int)(c.pk.ws_plane[l] * 2);   // bytes per plane (gemm_split)
    y.wf32 = c.packed + c.pk.wf_off[l];
    y.bias = c.params + c.L.bias_off[l];
    y.out = store_act ? c.at<float>(c.P.in_off[l + 1]) : nullptr;
    y.ld_out = c.P.ld_in[l + 1];
    y.in = c.net->in_dim[l]; y.out_dim = c.net->out_dim[l]; y.U = c.pk.uf[l];
    const Drop drop = drop_of(c.net, l, c.training);
    if (drop.on) { y.drop_thr = drop.thr; y.drop_key = c.keys[l]; y.drop_scale = drop.scale; }
    y.x0_col = ((c.net->skip_mask >> (l + 1)) & 1) ? c.net->out_dim[l] : -1;
    y.maskbits = store_act ? c.at<uint32_t>(c.P.mask_off[l]) : nullptr;
    if (seg != nullptr) {   // hoisted x0 columns: nothing left to contract for layer 0, only the previous layer for the skip layer
      y.x0_col = -1;
      if (l == 0) y.in = 0;
      else if ((c.net->skip_mask >> l) & 1) y.in = c.net->out_dim[l - 1];
    }
  }
  if (seg != nullptr) a.seg = *seg;
  a.w_last = c.packed + c.pk.w_off[last]; a.b_last = c.params + c.L.bias_off[last]; a.in_last = c.net->in_dim[last];
  a.use_tanh = c.net->use_tanh; a.y_out = y_out; a.u_out = u_out;
  if (defer != nullptr) {
    a.ly[last - 1].out = nullptr;   // the last hidden activation is consumed from the slab by the backward head: no global copy
    *defer = a;
    return 0;
  }
  double wmac = 0;
  for (int l = 0; l < last; ++l) wmac += (double)c.net->in_dim[l] * c.net->out_dim[l];
  ProfScope ps(DSDF_PROF_FUSED_FWD, 2.0 * (double)c.n * wmac, c.st);
#ifdef DSDF_LAB
  static LabStamps stamps{"DSDF_LAB_DBG", 8192 * 64 * 8, false, nullptr};
  LabScope lab(stamps, c.st);
  a.dbg = stamps.dev;
#endif
  const FamilyKernels& k = KERNELS[c.path.family];
  const FwdKernel kernel = store_act ? k.fwd_act : k.fwd;
  if (kernel == nullptr) return fail(DSDF_E_LAUNCH, "internal: kernel family %d has no forward of its own", (int)c.path.family);
  const dim3 grid((unsigned)((c.n + c.P.frows - 1) / c.P.frows));
  hipLaunchKernelGGL(kernel, grid, dim3(store_act ? k.block : k.fwd_block), 0, c.st, a);
  LAUNCH_OK("fused_forward_kernel");
  return 0;
}

// hidden layers 0..nl-2: in[l+1][:, :out_l] = dropout(relu(in[l] W_l^T + b_l)); LayerNorm layers: Linear (bias) into the xhat
// buffer, then ln_fwd_kernel normalises in place (kept for the backward when save_ln) and writes the activated output
int run_hidden_forward(const Call& c, bool save_ln = true) {
  for (int l = 0; l < c.net->n_layers - 1; ++l) {
    NtArgs a;
    memset(&a, 0, sizeof(a));
    a.A = c.at<float>(c.P.in_off[l]); a.lda = c.P.ld_in[l];
    a.B = c.packed + c.pk.w_off[l]; a.ldb = c.pk.ldw[l];
    a.C = c.at<float>(c.P.in_off[l + 1]); a.ldc = c.P.ld_in[l + 1];
    a.M = (int)c.n; a.N = c.net->out_dim[l]; a.K = c.net->in_dim[l];
    a.bias = c.params + c.L.bias_off[l];
    a.relu = 1;
    const Drop drop = drop_of(c.net, l, c.training);
    if (ln_applied(c.net, l)) {
      a.C = c.at<float>(c.P.lnx_off[l]);
      TRY(launch_nt<EPI_PLAIN>(a, c.st));
      LnFwdArgs f;
      memset(&f, 0, sizeof(f));
      f.y = a.C; f.ldy = a.ldc; f.gamma = c.params + c.L.ln_w_off[l]; f.beta = c.params + c.L.ln_b_off[l];
      f.out = c.at<float>(c.P.in_off[l + 1]); f.ldo = c.P.ld_in[l + 1]; f.n = (int)c.n; f.width = c.net->out_dim[l];
      f.save = save_ln ? 1 : 0; f.rstd = save_ln ? c.at<float>(c.P.lnr_off[l]) : nullptr;
      if (drop.on) { f.drop_thr = drop.thr; f.drop_key = c.keys[l]; f.drop_scale = drop.scale; f.row_offset = c.row_offset; }
      hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((c.n + 3) / 4)), dim3(256), 0, c.st, f);
      LAUNCH_OK("ln_fwd_kernel");
      continue;
    }
    if (drop.on) { a.drop_thr = drop.thr; a.drop_key = c.keys[l]; a.drop_scale = drop.scale; a.row_offset = c.row_offset; }
    TRY(launch_nt<EPI_FWD>(a, c.st));
  }
  return 0;
}

struct FuseAdam { const DsdfAdamCfg* cfg; float* params; float* exp_avg; float* exp_avg_sq; float* packed; bool used; };

// Where a layer's weight gradient comes from: its split-K slabs and the column-sum partials that are its bias gradient
struct FinSrc { const float* slabs; int nsplit; long long slab; int ldc; const float* colsum; int npart; int ldcs; };
// One layer's finalize descriptor: slab sums, weight-norm backward and bias gradient into the gradient arena -- or, fz != nullptr
// (dsdf_train_step), consumed on the spot by Adam, which also writes the row's new weight-norm scale
// ... and where it goes: the gradient arena (added to what is there, or not), or straight into Adam
struct GradSink { float* grads; int accumulate; const FuseAdam* fz; };
FinArgs fin_args(const Call& c, int l, const FinSrc& src, const GradSink& to) {
  FinArgs f;
  memset(&f, 0, sizeof(f));
  f.slabs = src.slabs; f.nsplit = src.nsplit; f.slab = src.slab; f.ldc = src.ldc;
  f.colsum = src.colsum; f.npart = src.npart; f.ldcs = src.ldcs;
  f.g = c.L.g_off[l] >= 0 ? c.params + c.L.g_off[l] : nullptr;
  f.v = c.params + c.L.v_off[l];
  f.dg = c.L.g_off[l] >= 0 ? to.grads + c.L.g_off[l] : nullptr;
  f.dv = to.grads + c.L.v_off[l];
  f.db = to.grads + c.L.bias_off[l];
  f.out = c.net->out_dim[l]; f.in = c.net->in_dim[l]; f.accumulate = to.accumulate;
  if (to.fz != nullptr) {
    const DsdfAdamCfg* ad = to.fz->cfg;
    const double bc1 = 1.0 - pow((double)ad->beta1, (double)ad->step), bc2 = 1.0 - pow((double)ad->beta2, (double)ad->step);
    f.adam = 1;
    f.pb = to.fz->params + c.L.bias_off[l]; f.mb = to.fz->exp_avg + c.L.bias_off[l]; f.sb = to.fz->exp_avg_sq + c.L.bias_off[l];
    f.pv = to.fz->params + c.L.v_off[l];    f.mv = to.fz->exp_avg + c.L.v_off[l];    f.sv = to.fz->exp_avg_sq + c.L.v_off[l];
    if (c.L.g_off[l] >= 0) { f.pg = to.fz->params + c.L.g_off[l]; f.mg = to.fz->exp_avg + c.L.g_off[l]; f.sg = to.fz->exp_avg_sq + c.L.g_off[l]; }
    int r0 = 0;
    for (int q = 0; q < l; ++q) r0 += c.net->out_dim[q];
    f.scale_out = to.fz->packed + c.pk.scale_off + r0;
    f.omb1 = 1.0f - ad->beta1; f.b2 = ad->beta2; f.omb2 = 1.0f - ad->beta2;
    f.step_size = (float)((double)ad->lr_decoder / bc1); f.bc2_sqrt = (float)sqrt(bc2); f.eps = ad->eps;
  }
  return f;
}

// d_input [n][W0] = dzA (+ dzB): the x0 gradients of layer 0 and of the skip layer
int add_dz_to_input(const Call& c, bool used_dzB, float* d_input, int64_t ld_din) {
  const long long tot = (long long)c.n * c.P.W0;
  hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.st, c.at<float>(c.P.dzA_off), c.P.ldz,
                     used_dzB ? c.at<float>(c.P.dzB_off) : nullptr, c.P.ldz, d_input, (long long)ld_din, (int)c.n, c.P.W0);
  LAUNCH_OK("add2_kernel");
  return 0;
}

// The output layer's arguments every mode shares; callers add their mode's fields.  backward: and what the two backward modes
// (training, module) share -- dP of the last hidden layer and the per-block partials
LastArgs last_args(const Call& c, bool backward = false) {
  const int last = c.net->n_layers - 1;
  LastArgs a;
  memset(&a, 0, sizeof(a));
  a.a = c.at<float>(c.P.in_off[last]); a.lda = c.P.ld_in[last]; a.in = c.net->in_dim[last];
  a.w = c.packed + c.pk.w_off[last]; a.b = c.params + c.L.bias_off[last]; a.n = (int)c.n; a.use_tanh = c.net->use_tanh;
  if (!backward) return a;
  a.dp_prev = c.at<float>(c.P.dp_off[0]);
  a.lddp = c.P.ld_dp; a.mask_scale = mask_scale_of(c.net, last - 1, c.training);
  a.part_dw = c.at<float>(c.P.part_off); a.ld_part = c.P.ld_part;
  a.part_colsum = c.at<float>(c.P.part_off) + c.P.ld_in[last];
  a.part_db = c.at<float>(c.P.partdb_off); a.part_loss = c.at<float>(c.P.partloss_off);
  a.n_act = c.net->out_dim[last - 1];
  return a;
}

// shared backward over hidden layers, given dp of layer nl-2 in dp[0] and the last layer's partials.
// ncols_dz: how many leading x0 columns of d/dx0 are needed (L for training, W0 for the module path).
// c.keys / c.row_offset: latent_dropout nets mask the latent part of layer 0's dX (dzA) with the forward's hash.
// xyz_acc != nullptr (xyz_in_all, module path with d/d(input)): *xyz_acc = true when dxz_off[1] holds the sum of the xyz_in
// layers' d/d(xyz) (the caller adds it to the xyz columns of d_input).
int run_backward(const Call& c, const GradSink& to, int ncols_dz, bool* used_dzB, bool want_dw, bool* xyz_acc = nullptr) {
  const int last = c.net->n_layers - 1;
  // second stage of the last layer's partials
  if (want_dw) {
    const int w = c.P.ld_part;
    hipLaunchKernelGGL(reduce_rows_kernel, dim3((w + 63) / 64, LAST_GROUPS), dim3(256), 0, c.st,
                       ReduceRowsArgs{c.at<float>(c.P.part_off), c.P.last_blocks, c.P.ld_part, w, c.at<float>(c.P.part2_off), LAST_GROUPS});
    LAUNCH_OK("reduce_rows_kernel");
    const FinSrc src{c.at<float>(c.P.part2_off), LAST_GROUPS, c.P.ld_part, c.P.ld_part, c.at<float>(c.P.partdb_off), c.P.last_blocks, 1};
    const FinArgs f = fin_args(c, last, src, to);      // (out_dim[last] == 1: one block)
    hipLaunchKernelGGL(finalize_layer_kernel, dim3(1), dim3(256), 0, c.st, f);
    LAUNCH_OK("finalize_layer_kernel(last)");
    if ((c.net->ln_param_mask >> last) & 1) {   // bn module of the last Linear: created by the reference, never called: zero gradient
      LnGradArgs z;
      memset(&z, 0, sizeof(z));
      z.dgamma = to.grads + c.L.ln_w_off[last]; z.dbeta = to.grads + c.L.ln_b_off[last]; z.width = c.net->out_dim[last]; z.accumulate = to.accumulate; z.zero = 1;
      hipLaunchKernelGGL(ln_param_grad_kernel, dim3(1), dim3(64), 0, c.st, z);
      LAUNCH_OK("ln_param_grad_kernel(last)");
    }
  }
  *used_dzB = false;
  int cur = 0;
  for (int l = last - 1; l >= 0; --l) {
    float* dp = c.at<float>(c.P.dp_off[cur]);
    // column-sum partials of dp as it arrives (from the output layer's kernel or the next layer's dX epilogue)
    const float* cs_ptr = l == last - 1 ? c.at<float>(c.P.part2_off) + c.P.ld_in[last] : c.at<float>(c.P.colsum_off);
    int cs_n = l == last - 1 ? LAST_GROUPS : c.P.mt, cs_ld = l == last - 1 ? c.P.ld_part : c.P.ldcs;
    const bool ln = ln_applied(c.net, l);
    if (ln) {   // dp is d/dz (after LayerNorm): turn it into d/d(Linear output) in place; gamma / beta / bias partials
      LnBwdArgs b;
      memset(&b, 0, sizeof(b));
      b.dz = dp; b.ldz = c.P.ld_dp; b.xhat = c.at<float>(c.P.lnx_off[l]); b.ldx = c.P.ld_in[l + 1]; b.rstd = c.at<float>(c.P.lnr_off[l]);
      b.gamma = c.params + c.L.ln_w_off[l]; b.n = (int)c.n; b.width = c.net->out_dim[l];
      b.part_dgamma = c.at<float>(c.P.lnpg_off); b.part_db = c.at<float>(c.P.lnpb_off); b.ldp = c.P.ldcs;
      int blocks = (int)((c.n + 3) / 4);
      if (blocks > LN_BLOCKS) blocks = LN_BLOCKS;
      hipLaunchKernelGGL(ln_bwd_kernel, dim3(blocks), dim3(256), 0, c.st, b);
      LAUNCH_OK("ln_bwd_kernel");
      if (want_dw) {
        LnGradArgs g;
        memset(&g, 0, sizeof(g));
        g.part_dgamma = b.part_dgamma; g.nblk = blocks; g.ldp = b.ldp; g.cs = cs_ptr; g.ncs = cs_n; g.ldcs = cs_ld;
        g.dgamma = to.grads + c.L.ln_w_off[l]; g.dbeta = to.grads + c.L.ln_b_off[l]; g.width = c.net->out_dim[l]; g.accumulate = to.accumulate;
        hipLaunchKernelGGL(ln_param_grad_kernel, dim3((g.width + 255) / 256), dim3(256), 0, c.st, g);
        LAUNCH_OK("ln_param_grad_kernel");
      }
      cs_ptr = b.part_db; cs_n = blocks; cs_ld = b.ldp;     // the Linear's bias gradient = column sums of dy
    }
    // dW_l = dp^T in_l  (split-K slabs)
    if (want_dw) {
    TnArgs t;
    memset(&t, 0, sizeof(t));
    t.A = dp; t.lda = c.P.ld_dp; t.B = c.at<float>(c.P.in_off[l]); t.ldb = c.P.ld_in[l];
    t.C = c.at<float>(c.P.slab_off); t.ldc = c.P.ld_in[l]; t.M = c.net->out_dim[l]; t.N = c.net->in_dim[l]; t.K = (int)c.n;
    t.kchunk = c.P.kchunk; t.slab = c.P.slab;
    TRY(launch_tn(t, c.P.nsplit, c.st));
    const FinArgs f = fin_args(c, l, FinSrc{t.C, c.P.nsplit, c.P.slab, t.ldc, cs_ptr, cs_n, cs_ld}, to);
    hipLaunchKernelGGL(finalize_layer_kernel, dim3(f.out), dim3(256), 0, c.st, f);
    LAUNCH_OK("finalize_layer_kernel");
    }
    // dX
    NtArgs a;
    memset(&a, 0, sizeof(a));
    a.A = dp; a.lda = c.P.ld_dp; a.B = c.packed + c.pk.wt_off[l]; a.ldb = c.pk.ldwt[l];
    a.M = (int)c.n; a.K = c.net->out_dim[l];
    if (l > 0) {
      const bool skip = (c.net->skip_mask >> l) & 1;
      a.C = c.at<float>(c.P.dp_off[cur ^ 1]); a.ldc = c.P.ld_dp;
      a.act = c.at<float>(c.P.in_off[l]); a.ldact = c.P.ld_in[l];
      a.mask_cols = c.net->out_dim[l - 1];
      a.mask_scale = mask_scale_of(c.net, l - 1, c.training);
      const bool xyz_l = !skip && c.net->xyz_in_all;                 // this layer's input is [a || xyz]
      const bool want_xyz = xyz_l && xyz_acc != nullptr && ncols_dz > c.net->latent_size;
      a.N = skip ? (ncols_dz > 0 ? a.mask_cols + ncols_dz : a.mask_cols) : (xyz_l ? a.mask_cols + (want_xyz ? c.net->geom_dim : 0) : c.net->in_dim[l]);
      if (skip && ncols_dz > 0) { a.C2 = c.at<float>(c.P.dzB_off); a.ldc2 = c.P.ldz; a.c2_cols = ncols_dz; *used_dzB = true; }
      if (want_xyz) { a.C2 = c.at<float>(c.P.dxz_off[0]); a.ldc2 = 4; a.c2_cols = c.net->geom_dim; }
      a.colsum = c.at<float>(c.P.colsum_off); a.ldcs = c.P.ldcs;
      TRY(launch_nt<EPI_BWD>(a, c.st));
      if (want_xyz) {
        const long long tot = (long long)c.n * c.net->geom_dim;
        hipLaunchKernelGGL(acc_cols_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.st, c.at<float>(c.P.dxz_off[0]), 4,
                           c.at<float>(c.P.dxz_off[1]), 4, 0, (int)c.n, c.net->geom_dim, *xyz_acc ? 1 : 0);
        LAUNCH_OK("acc_cols_kernel");
        *xyz_acc = true;
      }
      cur ^= 1;
    } else if (ncols_dz > 0) {
      a.C = c.at<float>(c.P.dzA_off); a.ldc = c.P.ldz; a.N = ncols_dz;
      TRY(launch_nt<EPI_PLAIN>(a, c.st));
      if (c.net->latent_dropout && c.training && c.keys != nullptr && c.net->latent_size > 0) {   // layer 0 saw the DROPPED latent
        const long long tot = (long long)c.n * c.net->latent_size;
        hipLaunchKernelGGL(latent_drop_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.st, c.at<float>(c.P.dzA_off), c.P.ldz,
                           (int)c.n, c.net->latent_size, c.keys[LATENT_DROPOUT_KEY], latent_drop_thr(), 1.0f / (1.0f - LATENT_DROPOUT_P), c.row_offset);
        LAUNCH_OK("latent_drop_bwd_kernel");
      }
    }
  }
  return 0;
}

// Backward with the fused dX chain (fused.hpp): ONE launch for the whole dX chain (writes every dP_l, column sums, latent-gradient
// inputs; merged with the forward in training), the second stage of the head's partials, then all dW (split-K) in one launch and all
// finalizes in one.  Five jobs, five functions, sequenced by run_backward_fused below.
// Segment mode (sb != nullptr): what the weight gradients of the hoisted layers need from the batch
struct SegBwd { const FusedSeg* seg; const int64_t* seg_scene; const float* table; int R;
                ScatterArgs* scatter; bool* scatter_done;       // the dense latent-gradient scatter may ride on the finalize launch
                                                                // (scatter->nslice is set there: the latent role decides it)
                const float* zr; };   // the segments' renormed latent rows (run_hoist), or nullptr: read table[seg_scene[r]]

// the layers whose dW + finalize a call of this phase does (DsdfLossCfg.dw_phase; 0: all)
inline bool in_phase(const Plan& P, int phase, int l) { return phase == 0 || (l >= P.dw_cut[phase] && l < P.dw_cut[phase - 1]); }

// (1) The dX chain's arguments: one descriptor per layer, deepest first (layer 0 only when d/dx0 is wanted: ncols_dz > 0)
FusedBwdArgs dx_chain_args(const Call& c, int ncols_dz, bool want_dw, const FusedBwdHead& head, const SegBwd* sb, bool* used_dzB) {
  const int last = c.net->n_layers - 1, ks = skip_layer(c.net);
  const bool segmode = sb != nullptr;
  *used_dzB = false;
  FusedBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.N = (int)c.n;
  a.head = head;
  if (segmode) { a.xyz = sb->seg->xyz; a.G = sb->seg->G; }
  int cnt = 0;
  for (int l = last - 1; l >= 0; --l) {
    if (l == 0 && ncols_dz <= 0) break;
    FusedBwdLayer& y = a.ly[cnt++];
    y.wtf = c.net->gemm_split ? c.packed + c.pk.wts_off[l] : c.packed + c.pk.wtf_off[l]; y.U = c.pk.utf[l]; y.K = c.net->out_dim[l];
    y.wplane = (int)(c.pk.wts_plane[l] * 2);
    y.wtf32 = c.packed + c.pk.wtf_off[l];
    if (l > 0) {
      const bool skip = (c.net->skip_mask >> l) & 1;
      y.mask_cols = c.net->out_dim[l - 1];
      y.mask_scale = mask_scale_of(c.net, l - 1, c.training);
      y.maskbits = c.at<uint32_t>(c.P.mask_off[l - 1]);
      y.dp_out = c.at<float>(c.P.dpl_off[l - 1]); y.ld_dp = c.P.ld_dp;
      y.colsum = c.at<float>(c.P.cs_off[l - 1]); y.ldcs = c.P.ldcs;
      if (segmode && want_dw && (l - 1 == 0 || l - 1 == ks)) y.xsum = c.at<float>(c.P.xsum_off[l - 1 == 0 ? 0 : 1]);
      if (segmode && l - 1 == 0) y.dp_out = nullptr;   // dP_0 is consumed through its column sums only
      if (skip && ncols_dz > 0) { y.dz_out = c.at<float>(c.P.dzB_off); y.ldz = c.P.ldz; y.dz_cols = ncols_dz; *used_dzB = true; }
      y.ncols = y.mask_cols + y.dz_cols;
    } else {
      y.mask_cols = 0; y.mask_scale = 1.f;
      y.dz_out = c.at<float>(c.P.dzA_off); y.ldz = c.P.ldz; y.dz_cols = ncols_dz; y.ncols = ncols_dz;
    }
  }
  a.n_layers = cnt;
  if (last_layer_skip(c.net)) {   // the head hands the x0 columns' gradient du w[x0 cols] to the skip-layer buffer of d/dx0
    a.head.dz_out = ncols_dz > 0 ? c.at<float>(c.P.dzB_off) : nullptr; a.head.ldz = c.P.ldz; a.head.dz_cols = ncols_dz;
    if (ncols_dz > 0) *used_dzB = true;
  }
  return a;
}

// (2) The dX chain's launch: merged with the deferred forward of the same points (fwd != nullptr), or the backward alone
int launch_dx_chain(const Call& c, FusedBwdArgs& a, const FusedFwdArgs* fwd) {
  // algorithmic FLOPs of the dX chain (the reference back-propagates through every hidden layer down to x0); the executed count is
  // smaller: layer 0's dX and the skip layer's x0 columns come from column sums instead
  double amac = 0;
  for (int l = 0; l < c.net->n_layers - 1; ++l) amac += (double)c.net->in_dim[l] * c.net->out_dim[l];
  const FamilyKernels& k = KERNELS[c.path.family];
  const dim3 grid((unsigned)c.P.nwg), block(k.block);
  if (fwd != nullptr) {
    if (k.fwd_bwd == nullptr) return fail(DSDF_E_LAUNCH, "internal: kernel family %d has no merged forward + backward", (int)c.path.family);
#ifdef DSDF_LAB
    // lab: stamps of the MERGED launch (forward slots 0.., backward slots 32..), dumped after every launch
    static LabStamps stamps{"DSDF_LAB_MDBG", 8192 * 64 * 8, true, nullptr};
    LabScope lab(stamps, c.st);
    FusedFwdArgs fwd_l = *fwd;
    if (stamps.dev) { fwd_l.dbg = stamps.dev; a.dbg = stamps.dev; fwd = &fwd_l; }
#endif
    ProfScope ps(DSDF_PROF_FUSED_FWD_BWD, 4.0 * (double)c.n * amac, c.st);   // forward + dX chain
    hipLaunchKernelGGL(k.fwd_bwd, grid, block, 0, c.st, *fwd, a);
    LAUNCH_OK("fused_fwd_bwd_kernel");
    return 0;
  }
  ProfScope ps(DSDF_PROF_FUSED_BWD, 2.0 * (double)c.n * amac, c.st);
  if (c.path.frows != FROWS || k.bwd == nullptr)
    return fail(DSDF_E_LAUNCH, "internal: the separate backward kernel has 64-row workgroups only");
  hipLaunchKernelGGL(k.bwd, grid, block, 0, c.st, a);
  LAUNCH_OK("fused_backward_kernel");
  return 0;
}

// (3) Segment mode: everything that consumes only the backward's per-workgroup partials (kernels.hpp post_bwd_role) -- run by
// the workgroups the dW launch leaves idle (rides), or by a launch of its own when there is no dW launch / no idle workgroup.
// Decides, launches nothing.
struct Roles {
  ReduceRowsArgs rr; int rr_bx;      // second stage of the head's per-workgroup partials (general mode: a launch of its own)
  PostBwdArgs q; int lat_n;          // segment mode: the role blocks, lat_n of them latent-gradient blocks
  int lat_slices;                    //   slices of a segment's latent gradient the scatter has to add
  int cus, dw_items, dw_busy;        // the dW launch: its items and the workgroups they keep busy
  bool rides;
};
Roles plan_roles(const Call& c, const DwSched& DS, bool want_dw, const SegBwd* sb, int phase) {
  const int ks = skip_layer(c.net);
  const bool segmode = sb != nullptr;
  Roles R;
  memset(&R, 0, sizeof(R));
  R.rr = ReduceRowsArgs{c.at<float>(c.P.part_off), c.P.nwg, c.P.ld_part, c.P.ld_part, c.at<float>(c.P.part2_off), LAST_GROUPS};
  R.rr_bx = (c.P.ld_part + 63) / 64;
  R.lat_slices = 1;
  PostBwdArgs& q = R.q;
  if (segmode) {
    if (want_dw) {
      q.rr = R.rr; q.rr_bx = R.rr_bx; q.rr_n = R.rr_bx * LAST_GROUPS;
      SegDwArgs& d = q.dw;
      d.nh = ks > 0 ? 2 : 1;
      d.cs[0] = c.at<float>(c.P.cs_off[0]); d.xsum[0] = c.at<float>(c.P.xsum_off[0]); d.out[0] = c.net->out_dim[0];
      if (ks > 0) { d.cs[1] = c.at<float>(c.P.cs_off[ks]); d.xsum[1] = c.at<float>(c.P.xsum_off[1]); d.out[1] = c.net->out_dim[ks]; }
      d.ldcs = c.P.ldcs; d.nwg = c.P.nwg; d.wg_per_seg = sb->seg->wg_per_seg; d.R = sb->R; d.L = c.net->latent_size; d.G = c.net->geom_dim;
      d.seg_scene = sb->seg_scene; d.table = sb->table; d.zr = sb->zr;
      d.HS = c.at<float>(c.P.hs_off); d.ldh = c.P.ldh; d.hstride = c.P.hstride;
      // (block counts of the launch-of-its-own form; the riding form below has its own)
      q.dw_n = (d.out[0] + SDW_ROWS_WIDE - 1) / SDW_ROWS_WIDE + (ks > 0 ? (d.out[1] + SDW_ROWS_WIDE - 1) / SDW_ROWS_WIDE : 0);
      if (seg_dw_long_form(d.wg_per_seg, d.out[0], d.out[1])) q.dw_n = d.out[0] + d.out[1];      // long segments, narrow layers: one row per block (seg_dw_row_body)
    }
    SegLatArgs& g = q.lat;   // per-segment latent gradient from the column sums of dP_0 / dP_skip
    g.cs0 = c.at<float>(c.P.cs_off[0]); g.ldcs = c.P.ldcs; g.out0 = c.net->out_dim[0];
    g.W0 = c.packed + c.pk.w_off[0]; g.ldw0 = c.pk.ldw[0];
    if (ks > 0) {
      g.csk = c.at<float>(c.P.cs_off[ks]); g.outk = c.net->out_dim[ks];
      g.Wk = c.packed + c.pk.w_off[ks]; g.ldwk = c.pk.ldw[ks]; g.koff = c.net->out_dim[ks - 1];
    }
    g.wg_per_seg = sb->seg->wg_per_seg; g.R = sb->R; g.L = c.net->latent_size;
    g.seg_scene = sb->seg_scene; g.table = sb->table; g.zr = sb->zr;
    g.segpart = c.at<float>(c.P.segpart_off); g.segnorm = c.at<float>(c.P.segnorm_off);
    q.lat_bx = sb->R;
    g.nchunk = (c.net->latent_size + 15) / 16;
    R.lat_n = sb->R * g.nchunk;
    // few long segments in a launch of their own (config 4: one shape): cut each segment's workgroups into slices so that the launch
    // has blocks for the chip; the scatter adds the slices
    g.nslice = 1; g.slice_stride = (long long)sb->R * c.net->latent_size;
    while (g.nslice < LAT_SLICES_MAX && R.lat_n * g.nslice * 2 <= chip_waves() / 4 && g.wg_per_seg / (g.nslice * 2) >= 16) g.nslice *= 2;
    R.lat_n *= g.nslice;
    R.lat_slices = g.nslice;
  }
  R.cus = chip_waves() / 4;
  R.dw_items = DS.n_full + DS.n_narrow;
  R.dw_busy = want_dw ? ((R.dw_items + 3) / 4 < R.cus ? (R.dw_items + 3) / 4 : R.cus) : 0;
  // the idle workgroups take the role blocks one after the other: that stays inside the dW time for batches of up to one
  // workgroup per CU (measured: 16384 points, 1168 role blocks on 16 workgroups, dW time unchanged); larger batches put
  // the roles on the critical path (65536 points: -5 %), so they get their own (wide) launch there
  static const bool no_ride = [] { const char* e = getenv("DSDF_NO_RIDE"); return e && e[0] == '1'; }();   // A/B switch
  // Round 4: stamps inside the launch (profiles/r04_dw_stamps_before.log) showed the riding roles to be its TAIL -- 391 us of role
  // blocks on the 16 spare workgroups against 377 us of MFMA items -- and their latency-bound chains to be what made the launch
  // 388 us on one box and 403 us on the next.  The roles were rebuilt for few workgroups (seg_dw_body: 32 rows per block;
  // seg_latgrad_all_body: one block per 16 latent columns takes all segments): they now end 242 us into the launch.
  // (gemm_split: measured again with the rebuilt roles -- they end 242 us into the launch, the split items 174 us: riding there made
  // the launch 253 us instead of 174 + 18 for a launch of their own, so they still do not ride in split mode)
  R.rides = segmode && want_dw && R.cus - R.dw_busy >= 8 && c.P.nwg <= R.cus && !no_ride && !c.net->gemm_split && phase <= 1 &&
            R.dw_items > 0;
  if (R.rides) {   // the few-workgroups forms: 32 weight-gradient rows per block, one latent-gradient block per 16 columns
    q.lat.nslice = 1; R.lat_slices = 1;
    q.lat_bx = 0;
    R.lat_n = (c.net->latent_size + 15) / 16;
    q.rr_n = q.rr_bx;               // one block per 64-column strip of the head's partials takes all groups (reduce_rows_strip_body)
    q.dw_n = (q.dw.out[0] + SDW_ROWS_RIDE - 1) / SDW_ROWS_RIDE + (ks > 0 ? (q.dw.out[1] + SDW_ROWS_RIDE - 1) / SDW_ROWS_RIDE : 0);
  }
  return R;
}

// (4) All dW_l = dP_l^T a_l (of this phase's layers) in one launch; the riding roles go to the workgroups its items leave idle
int launch_dw(const Call& c, const DwSched& DS, const Roles& R, bool segmode, int phase) {
  const int last = c.net->n_layers - 1;
  DwArgs d;
  memset(&d, 0, sizeof(d));
  d.n_layers = last; d.n_full = DS.n_full; d.n_narrow = DS.n_narrow; d.N = (int)c.n;
  double fl = 0;
  for (int l = 0; l < last; ++l) {
    DwLayer& y = d.ly[l];
    y.dp = c.at<float>(c.P.dpl_off[l]); y.ld_dp = c.P.ld_dp;
    y.act = c.at<float>(c.P.in_off[l]); y.ld_act = c.P.ld_in[l];
    y.slabs = c.at<float>(c.P.dwslab_off[l]); y.slab = DS.slab[l];
    y.M = c.net->out_dim[l]; y.Nc = dw_cols(c.net, l, segmode); y.ldc = c.P.ld_in[l];
    y.tiles_m = DS.tiles_m[l]; y.tiles_n = DS.tiles_n[l]; y.last_nj = DS.last_nj[l]; y.nfull_n = DS.nfull_n[l];
    y.nsplit = DS.nsplit[l]; y.kchunk = DS.kchunk[l]; y.full0 = DS.full0[l]; y.narrow0 = DS.narrow0[l];
    if (in_phase(c.P, phase, l)) fl += 2.0 * (double)c.n * y.M * c.net->in_dim[l];   // algorithmic (segment mode executes fewer: hoisted x0 columns)
  }
#ifdef DSDF_LAB
  static LabStamps stamps{"DSDF_LAB_DWDBG", 1024 * 4 * 8 * 8, true, nullptr};      // lab: per-wave stamps of the LAST dW launch, dumped at every launch
  LabScope lab(stamps, c.st);
  d.dbg = stamps.dev;
#endif
  ProfScope ps(DSDF_PROF_DW_STREAM, fl, c.st);
  const DwKernel kernel = KERNELS[c.path.family].dw;
  if (R.rides) {
    hipLaunchKernelGGL(kernel, dim3(R.cus), dim3(256), 0, c.st, d, R.q, R.lat_n, R.dw_busy);
  } else {
    PostBwdArgs none;
    memset(&none, 0, sizeof(none));
    const int grid = R.dw_busy < 1 ? 1 : R.dw_busy;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, c.st, d, none, 0, grid);
  }
  LAUNCH_OK("dw_stream_kernel");
  return 0;
}

// (5) The finalize table: split-K sums, weight-norm backward and bias gradients [+ Adam] of ALL of this phase's layers (last layer
// included), one launch.  Returns the launch's block count (0: an empty bucket -- fewer layers than buckets).
int fin_table(const Call& c, const DwSched& DS, const GradSink& to, bool segmode, int phase, FinAll* fa) {
  const int last = c.net->n_layers - 1, ks = skip_layer(c.net);
  memset(fa, 0, sizeof(*fa));
  int rows = 0;      // counts BLOCKS of the finalize launch
  for (int l = last; l >= 0; --l) {
    if (!in_phase(c.P, phase, l)) continue;
    FinSrc src;
    if (l == last) src = FinSrc{c.at<float>(c.P.part2_off), LAST_GROUPS, c.P.ld_part, c.P.ld_part, c.at<float>(c.P.partdb_off), c.P.nwg, 1};
    else if (l == last - 1)
      src = FinSrc{c.at<float>(c.P.dwslab_off[l]), DS.nsplit[l], DS.slab[l], c.P.ld_in[l], c.at<float>(c.P.part2_off) + c.P.ld_in[last], LAST_GROUPS, c.P.ld_part};
    else src = FinSrc{c.at<float>(c.P.dwslab_off[l]), DS.nsplit[l], DS.slab[l], c.P.ld_in[l], c.at<float>(c.P.cs_off[l]), c.P.nwg, c.P.ldcs};
    FinArgs& f = fa->f[fa->n];
    f = fin_args(c, l, src, to);
    if (segmode && (l == 0 || l == ks)) {
      f.hoist = 1; f.lat0 = l == 0 ? 0 : c.net->out_dim[l - 1]; f.hW = c.net->latent_size + c.net->geom_dim; f.ldh = c.P.ldh;
      f.hs = c.at<float>(c.P.hs_off) + (l == 0 ? 0 : c.P.hstride);
    }
    fa->row0[fa->n] = rows;
    rows += fin_blocks(f.out, f.in);
    ++fa->n;
  }
  fa->row0[fa->n] = rows;
  return rows;
}

// fwd: the deferred forward of the same points -> one launch for both.
// phase (DsdfLossCfg.dw_phase): 0 = everything; p >= 1: dW + finalize of bucket p - 1 only (p = 1: after the forward + backward launch
// and its roles)
int run_backward_fused(const Call& c, const GradSink& to, int ncols_dz, bool* used_dzB, bool want_dw, const FusedBwdHead& head,
                       const SegBwd* sb, const FusedFwdArgs* fwd, int phase) {
  const DwSched& DS = phase == 0 ? c.P.dw : c.P.dwph[phase - 1];
  const bool segmode = sb != nullptr;
  FusedBwdArgs a = dx_chain_args(c, ncols_dz, want_dw, head, sb, used_dzB);
  if (phase <= 1) TRY(launch_dx_chain(c, a, fwd));
  const Roles R = plan_roles(c, DS, want_dw, sb, phase);
  if (!segmode && phase <= 1 && want_dw) {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3(R.rr_bx, LAST_GROUPS), dim3(256), 0, c.st, R.rr);
    LAUNCH_OK("reduce_rows_kernel");
  }
  if (segmode && sb->scatter != nullptr) { sb->scatter->nslice = R.lat_slices; sb->scatter->slice_stride = (long long)sb->R * c.net->latent_size; }
  if (segmode && !R.rides && phase <= 1) {
    hipLaunchKernelGGL(post_bwd_kernel, dim3((unsigned)(R.q.rr_n + R.q.dw_n + R.lat_n)), dim3(256), 0, c.st, R.q, R.lat_n);
    LAUNCH_OK("post_bwd_kernel");
  }
  if (!want_dw) return 0;
  if (R.dw_items > 0) TRY(launch_dw(c, DS, R, segmode, phase));
  FinAll fa;
  const int rows = fin_table(c, DS, to, segmode, phase, &fa);
  if (rows == 0) return 0;
  if (segmode && sb->scatter != nullptr && phase <= 1) {   // the dense latent-gradient scatter rides on the finalize launch
    hipLaunchKernelGGL(finalize_scatter_kernel, dim3(rows + sb->R), dim3(256), 0, c.st, fa, *sb->scatter, rows);
    LAUNCH_OK("finalize_scatter_kernel");
    *sb->scatter_done = true;
  } else {
    hipLaunchKernelGGL(finalize_all_kernel, dim3(rows), dim3(256), 0, c.st, fa);
    LAUNCH_OK("finalize_all_kernel");
  }
  return 0;
}

FusedBwdHead make_head(const Call& c, int mode) {
  const int last = c.net->n_layers - 1;
  FusedBwdHead h;
  memset(&h, 0, sizeof(h));
  h.mode = mode;
  h.a_last = c.at<float>(c.P.in_off[last]); h.ld_a = c.P.ld_in[last]; h.in_last = c.net->in_dim[last];
  h.w_last = c.packed + c.pk.w_off[last]; h.b_last = c.params + c.L.bias_off[last]; h.use_tanh = c.net->use_tanh;
  h.mask_scale = mask_scale_of(c.net, last - 1, c.training);
  h.dp_out = c.at<float>(c.P.dpl_off[last - 1]); h.ld_dp = c.P.ld_dp;
  h.part = c.at<float>(c.P.part_off); h.ld_part = c.P.ld_part;
  h.part_db = c.at<float>(c.P.partdb_off); h.part_loss = c.at<float>(c.P.partloss_off);
  h.n_act = c.net->out_dim[last - 1];      // (< in_last only when latent_in names the output layer: run_backward_fused points dz_out)
  return h;
}

// The opening of every entry point that launches the decoder, in the order a caller can observe through the error it gets:
//   switches -> the checks all of them share -> n == 0 is a no-op (training excepted: an empty batch is an error of its own) ->
//   own(), the entry's argument checks (net is valid and c.path picked by then) -> layouts -> lay(c), the workspace plan for
//   c.path (recording t_last_plan) -> the size check against its total.
// Returns 0 with c filled, or the error; after a 0 the caller returns at once when n == 0.  training / keys / row_offset stay zero.
template <class Own, class Lay>
int open_call(Call& c, Entry entry, const DsdfNet* net, const float* packed, const float* params, void* ws, size_t ws_bytes,
              void* stream, int64_t n, Own own, Lay lay) {
  memset(&c, 0, sizeof(c));
  c.sw = Switches::read();
  TRY(validate(net));
  // (validate() admits fwd_bf16 / gemm_split only for nets the fused kernels cover: without them the switch is the one reason)
  const bool fused = pick_path(net, 0, ENTRY_MODULE_FWD, c.sw).fused;
  if (net->fwd_bf16 && !fused) return fail(DSDF_E_INVALID, "fwd_bf16 exists only in the fused kernels (DSDF_NO_FUSED is set)");
  if (net->gemm_split && !fused) return fail(DSDF_E_INVALID, "gemm_split exists only in the fused kernels (DSDF_NO_FUSED is set)");
  if (!packed || !params || !ws) return fail(DSDF_E_INVALID, "NULL packed/params/workspace pointer");
  if (!aligned16(packed) || !aligned16(params) || (reinterpret_cast<uintptr_t>(ws) & 255))
    return fail(DSDF_E_INVALID, "packed/params must be 16-byte and workspace 256-byte aligned");
  if (n == 0 && entry != ENTRY_TRAIN) return 0;
  c.net = net; c.packed = packed; c.params = params; c.ws = ws; c.n = n; c.st = (hipStream_t)stream;
  c.path = pick_path(net, n, entry, c.sw);
  TRY(own());
  param_layout(net, &c.L);
  c.pk = packed_layout(net);
  c.P = lay(c);
  if (ws_bytes < c.P.total) return fail(DSDF_E_WORKSPACE, "workspace %zu < %zu bytes", ws_bytes, c.P.total);
  return 0;
}
// ... with the layout of a call without segments or buckets: the inference plan or the module path's, for the path's rows (or frows)
template <class Own>
int open_call(Call& c, Entry entry, const DsdfNet* net, const float* packed, const float* params, void* ws, size_t ws_bytes,
              void* stream, int64_t n, Own own, int frows = 0) {
  return open_call(c, entry, net, packed, params, ws, ws_bytes, stream, n, own, [=](const Call& c) {
    return make_plan(c.net, c.n, 0, entry == ENTRY_INFER, false, 2, frows ? frows : c.path.frows, &t_last_plan);
  });
}

}  // namespace

// ===================================================================================================
extern "C" {

int dsdf_abi_version(void) { return DSDF_ABI_VERSION; }
const char* dsdf_last_error(void) { return g_err; }

int dsdf_param_layout(const DsdfNet* net, DsdfParamLayout* out) {
  TRY(validate(net));
  if (!out) return fail(DSDF_E_INVALID, "out is NULL");
  param_layout(net, out);
  return 0;
}

int dsdf_packed_floats(const DsdfNet* net, int64_t* n_floats) {
  TRY(validate(net));
  if (!n_floats) return fail(DSDF_E_INVALID, "n_floats is NULL");
  *n_floats = packed_layout(net).total;
  return 0;
}

int dsdf_workspace_bytes_buckets(const DsdfNet* net, int64_t n_points, int64_t n_segments, int32_t n_buckets, size_t* bytes) {
  TRY(validate(net));
  if (!bytes || n_points < 0 || n_segments < 0) return fail(DSDF_E_INVALID, "bad arguments");
  if (n_points > (1ll << 30)) return fail(DSDF_E_INVALID, "n_points too large");
  if (n_buckets < 0 || n_buckets > DSDF_MAX_BUCKETS) return fail(DSDF_E_INVALID, "n_buckets %d out of range [0, %d]", n_buckets, DSDF_MAX_BUCKETS);
  size_t best = 0;
  for (int fr = 32; fr <= FROWS; fr += 32)      // (32-row workgroups double the per-workgroup partials: pick_path decides per call)
    for (int seg = 0; seg < 2; ++seg)           // segment mode lays the workspace out differently
      best = std::max(best, make_plan(net, n_points, n_segments, false, seg != 0, n_buckets, fr).total);
  *bytes = best;
  return 0;
}

int dsdf_workspace_bytes(const DsdfNet* net, int64_t n_points, int64_t n_segments, size_t* bytes) {
  return dsdf_workspace_bytes_buckets(net, n_points, n_segments, 2, bytes);
}

int dsdf_dw_phase_supported(const DsdfNet* net) {
  TRY(validate(net));
  return pick_path(net, 0, ENTRY_TRAIN, Switches::read()).fused ? 1 : 0;
}

int dsdf_grad_buckets(const DsdfNet* net, int32_t n_buckets, int32_t* first_layer, int64_t* arena_off) {
  TRY(validate(net));
  if (!first_layer || !arena_off) return fail(DSDF_E_INVALID, "NULL argument");
  if (n_buckets < 2 || n_buckets > DSDF_MAX_BUCKETS) return fail(DSDF_E_INVALID, "n_buckets %d out of range [2, %d]", n_buckets, DSDF_MAX_BUCKETS);
  DsdfParamLayout L;
  param_layout(net, &L);
  int cut[DSDF_MAX_BUCKETS + 1];
  dw_bucket_cuts(net, n_buckets, cut);
  auto layer_start = [&](int k) {              // a layer's parameters are one contiguous block: its first offset
    if (k >= net->n_layers) return L.total;
    int64_t o = L.v_off[k];
    if (L.bias_off[k] >= 0 && L.bias_off[k] < o) o = L.bias_off[k];
    if (L.g_off[k] >= 0 && L.g_off[k] < o) o = L.g_off[k];
    if (L.ln_w_off[k] >= 0 && L.ln_w_off[k] < o) o = L.ln_w_off[k];
    return o;
  };
  arena_off[0] = L.total;                      // bucket b = layers [first_layer[b], ...) = arena floats [arena_off[b + 1], arena_off[b])
  for (int b = 0; b < n_buckets; ++b) { first_layer[b] = cut[b + 1]; arena_off[b + 1] = layer_start(cut[b + 1]); }
  return 0;
}

int dsdf_decode_workspace_bytes(const DsdfNet* net, int64_t n_points, size_t* bytes) {
  TRY(validate(net));
  if (!bytes || n_points < 0 || n_points > (1ll << 30)) return fail(DSDF_E_INVALID, "bad arguments");
  *bytes = make_plan(net, n_points, 0, true).total;
  return 0;
}

int dsdf_materialize_weights(const DsdfNet* net, const float* params, float* packed, void* stream) {
  TRY(validate(net));
  if (!params || !packed) return fail(DSDF_E_INVALID, "NULL pointer");
  return materialize(net, params, packed, (hipStream_t)stream);
}

int dsdf_decode(const DsdfNet* net, const float* packed, const float* params, const float* input, int64_t ld_in,
                int64_t n, float* sdf_out, void* ws, size_t ws_bytes, void* stream) {
  Call c;
  const int rc = open_call(c, ENTRY_INFER, net, packed, params, ws, ws_bytes, stream, n, [&] {
    return !input || !sdf_out || n < 0 || ld_in < net->in_dim[0] ? fail(DSDF_E_INVALID, "bad input/sdf_out/ld_in") : 0;
  });
  if (rc != 0 || n == 0) return rc;
  TRY(run_gather(c, nullptr, nullptr, input, ld_in));
  if (c.path.fused) return run_fused_forward(c, false, sdf_out, nullptr);
  TRY(run_hidden_forward(c, false));
  LastArgs a = last_args(c);
  a.y_out = sdf_out;
  int blocks = (int)((n + 15) / 16);
  if (blocks > 2048) blocks = 2048;
  return launch_last<LAST_FWD>(a, blocks, c.st);
}

// dsdf_decode_latent's own layout: the one-row "scene table" index and U [1][2][FMAXW] behind it.  The caller's buffer is still
// sized like dsdf_decode's (at least 16384 bytes: the plan's total); none of that plan's regions is touched.
static Plan decode_latent_plan(const DsdfNet* net, int64_t n, int frows, size_t* scene_off, WsTable* rec) {
  Plan P = make_plan(net, n, 0, true, false, 2, frows);
  WsCarver c(rec);
  *scene_off = c.take("dl_scene", -1, 8);                                             // seg_scene[0] = 0: the "table" is the single latent row
  P.hoistU_off = c.take("dl_hoistU", -1, (size_t)2 * FMAXW * 4); P.ldu = FMAXW;      // U [1][2][512] behind it
  P.total = c.finish(std::max(std::max<size_t>(P.total, 16384), c.o));
  return P;
}

static bool decode_latent_ok(const DsdfNet* net, const Path& path) {
  return path.fused && net->geom_dim <= FGEO && net->latent_size <= HOIST_MAXL &&
         net->latent_size >= 1 && net->n_layers >= 3 && !last_layer_skip(net);
}

int dsdf_decode_latent_supported(const DsdfNet* net) {
  TRY(validate(net));
  return decode_latent_ok(net, pick_path(net, 0, ENTRY_INFER, Switches::read())) ? 1 : 0;
}

int dsdf_decode_latent(const DsdfNet* net, const float* packed, const float* params, const float* latent, const float* xyz,
                       int64_t n, float* sdf_out, void* ws, size_t ws_bytes, void* stream) {
  Call c;
  size_t scene_off = 0;
  const int rc = open_call(
      c, ENTRY_INFER, net, packed, params, ws, ws_bytes, stream, n,
      [&] {
        if (!latent || !xyz || !sdf_out || n < 0) return fail(DSDF_E_INVALID, "bad latent/xyz/sdf_out");
        if (!decode_latent_ok(net, c.path))
          return fail(DSDF_E_INVALID, "dsdf_decode_latent needs the fused forward (widths <= 512, geom_dim <= 4): use dsdf_decode");
        return 0;
      },
      [&](const Call& c) { return decode_latent_plan(net, n, c.path.frows, &scene_off, &t_last_plan); });
  if (rc != 0 || n == 0) return rc;
  // ONE segment covering every point: the segment-mode forward with the latent's products hoisted (fused.hpp FusedSeg)
  HIP_OK(hipMemsetAsync(c.at<char>(scene_off), 0, 8, c.st));
  DsdfBatch b;
  memset(&b, 0, sizeof(b));
  b.seg_scene = c.at<int64_t>(scene_off); b.n_segments = 1; b.xyz = xyz; b.n_points = n; b.seg_len = n;
  FusedSeg seg;
  TRY(run_hoist(c, latent, &b, &seg));
  seg.wg_per_seg = (int)((n + c.P.frows - 1) / c.P.frows);  // every workgroup belongs to segment 0
  return run_fused_forward(c, false, sdf_out, nullptr, &seg);
}

// ---- debug only: red zones and the region table of the workspace planners (include/dsdf.h) ----------------
int dsdf_debug_ws_redzone(int32_t bytes) {
  if (bytes < 0 || bytes > DSDF_WS_MAX_REDZONE || (bytes & 255))
    return fail(DSDF_E_INVALID, "red zone of %d bytes: must be 0 or a multiple of 256, at most %d", bytes, DSDF_WS_MAX_REDZONE);
  g_redzone.store((size_t)bytes, std::memory_order_relaxed);
  return 0;
}

int dsdf_debug_ws_regions(DsdfWsRegion* table, int32_t capacity, int32_t* n_regions, size_t* total) {
  const WsTable& T = t_last_plan;
  if (!n_regions) return fail(DSDF_E_INVALID, "n_regions is NULL");
  *n_regions = T.n;
  if (total) *total = T.total;
  if (T.dropped) return fail(DSDF_E_INVALID, "the last plan has %d regions more than DSDF_WS_MAX_REGIONS", T.dropped);
  if (!table) return 0;                      // count / total only
  if (capacity < T.n) return fail(DSDF_E_INVALID, "table of %d rows, the last plan has %d regions", capacity, T.n);
  for (int i = 0; i < T.n; ++i) {
    memset(&table[i], 0, sizeof(table[i]));
    if (T.row[i].idx >= 0) snprintf(table[i].name, sizeof(table[i].name), "%s%d", T.row[i].name, T.row[i].idx);
    else snprintf(table[i].name, sizeof(table[i].name), "%s", T.row[i].name);
    table[i].offset = T.row[i].off; table[i].bytes = T.row[i].bytes;
  }
  return 0;
}

int dsdf_debug_ws_plan(const DsdfNet* net, int64_t n_points, int64_t n_segments, int32_t kind, int32_t segmode, int32_t n_buckets,
                       int32_t frows) {
  TRY(validate(net));
  if (n_points < 0 || n_points > (1ll << 30) || n_segments < 0) return fail(DSDF_E_INVALID, "bad arguments");
  if (frows != 32 && frows != FROWS) return fail(DSDF_E_INVALID, "frows %d: the fused kernels take 32 or %d rows", frows, FROWS);
  if (n_buckets < 0 || n_buckets > DSDF_MAX_BUCKETS) return fail(DSDF_E_INVALID, "n_buckets %d out of range [0, %d]", n_buckets, DSDF_MAX_BUCKETS);
  switch (kind) {
    case DSDF_WS_PLAN_TRAIN: make_plan(net, n_points, n_segments, false, segmode != 0, n_buckets, frows, &t_last_plan); return 0;
    case DSDF_WS_PLAN_DECODE: make_plan(net, n_points, 0, true, false, 2, frows, &t_last_plan); return 0;
    case DSDF_WS_PLAN_DECODE_LATENT: {
      size_t scene_off = 0;
      decode_latent_plan(net, n_points, frows, &scene_off, &t_last_plan);
      return 0;
    }
    default: return fail(DSDF_E_INVALID, "plan kind %d", kind);
  }
}

int dsdf_debug_packed_layout(const DsdfNet* net, DsdfPackedLayout* out) {
  TRY(validate(net));
  if (!out) return fail(DSDF_E_INVALID, "out is NULL");
  const Packed pk = packed_layout(net);
  out->total = pk.total; out->scale_off = pk.scale_off;
  for (int l = 0; l < DSDF_MAX_LAYERS; ++l) {
    const bool in = l < net->n_layers;
    out->w_off[l] = in ? pk.w_off[l] : -1;     out->wt_off[l] = in ? pk.wt_off[l] : -1;
    out->wf_off[l] = in ? pk.wf_off[l] : -1;   out->wtf_off[l] = in ? pk.wtf_off[l] : -1;
    out->wfb_off[l] = in ? pk.wfb_off[l] : -1;
    out->ws_off[l] = in ? pk.ws_off[l] : -1;   out->wts_off[l] = in ? pk.wts_off[l] : -1;
    out->ws_plane[l] = in ? pk.ws_plane[l] : 0; out->wts_plane[l] = in ? pk.wts_plane[l] : 0;
    out->ldw[l] = in ? pk.ldw[l] : 0; out->ldwt[l] = in ? pk.ldwt[l] : 0;
    out->uf[l] = in ? pk.uf[l] : 0;   out->utf[l] = in ? pk.utf[l] : 0;
  }
  return 0;
}

int dsdf_module_forward(const DsdfNet* net, const float* packed, const float* params, const float* input,
                        int64_t ld_in, int64_t n, int32_t training, const uint32_t* dropout_key, float* sdf_out,
                        void* ws, size_t ws_bytes, void* stream) {
  Call c;
  const int rc = open_call(c, ENTRY_MODULE_FWD, net, packed, params, ws, ws_bytes, stream, n, [&] {
    if (!input || !sdf_out || n < 0 || ld_in < net->in_dim[0]) return fail(DSDF_E_INVALID, "bad input/sdf_out/ld_in");
    if (training && net->dropout_p > 0.f && net->dropout_mask && !dropout_key) return fail(DSDF_E_INVALID, "dropout_key is NULL");
    return 0;
  });
  if (rc != 0 || n == 0) return rc;
  c.training = training; c.keys = dropout_key;
  TRY(run_gather(c, nullptr, nullptr, input, ld_in));
  if (c.path.fused) return run_fused_forward(c, true, sdf_out, c.at<float>(c.P.u_off));
  TRY(run_hidden_forward(c));
  LastArgs a = last_args(c);
  a.y_out = sdf_out; a.u_save = c.at<float>(c.P.u_off);
  return launch_last<LAST_FWD>(a, c.P.last_blocks, c.st);
}

// want_dw == false (dsdf_module_input_grad): the same launches without the weight-gradient ones; grads is not touched
static int module_backward_impl(const DsdfNet* net, const float* packed, const float* params, const float* d_sdf, int64_t n,
                                int32_t training, const uint32_t* dropout_key, float* grads, int32_t accumulate, float* d_input,
                                int64_t ld_din, void* ws, size_t ws_bytes, void* stream, bool want_dw) {
  Call c;
  const int rc = open_call(c, ENTRY_MODULE_BWD, net, packed, params, ws, ws_bytes, stream, n, [&] {
    if (!d_sdf || (want_dw && !grads) || n < 0) return fail(DSDF_E_INVALID, "bad d_sdf/grads");
    if (d_input && ld_din < net->in_dim[0]) return fail(DSDF_E_INVALID, "ld_din too small");
    if (training && net->latent_dropout && d_input && !dropout_key)
      return fail(DSDF_E_INVALID, "dropout_key is NULL (latent_dropout needs the forward's key for d/d(input))");
    return 0;
  });
  if (rc != 0 || n == 0) return rc;
  c.training = training; c.keys = dropout_key;
  const Plan& P = c.P;
  const GradSink to{grads, accumulate, nullptr};
  bool used_dzB = false;
  if (c.path.fused) {
    FusedBwdHead h = make_head(c, HEAD_EXT);
    h.d_sdf = d_sdf; h.u_in = c.at<float>(P.u_off);
    TRY(run_backward_fused(c, to, d_input ? P.W0 : 0, &used_dzB, want_dw, h, nullptr, nullptr, 0));
  } else {
    const int last = net->n_layers - 1;
    LastArgs a = last_args(c, true);
    a.d_sdf = d_sdf; a.u_in = c.at<float>(P.u_off);
    if (last_layer_skip(net) && d_input) { a.dz = c.at<float>(P.dzB_off); a.ldz = P.ldz; a.dz_cols = P.W0; }
    TRY(launch_last<LAST_BWD_EXT>(a, P.last_blocks, c.st));
    bool xyz_acc = false;
    if (d_input && net->xyz_in_all && last > 0) {   // the last layer's input is [a || xyz] too: its own d/d(xyz) opens the running sum
      const long long tot = (long long)n * net->geom_dim;
      hipLaunchKernelGGL(last_xyz_grad_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.st, d_sdf, c.at<float>(P.u_off),
                         packed + c.pk.w_off[last] + net->out_dim[last - 1], net->geom_dim, net->use_tanh, c.at<float>(P.dxz_off[1]), 4, 0,
                         (int)n, 0);
      LAUNCH_OK("last_xyz_grad_kernel");
      xyz_acc = true;
    }
    TRY(run_backward(c, to, d_input ? P.W0 : 0, &used_dzB, want_dw, (d_input && net->xyz_in_all) ? &xyz_acc : nullptr));
    if (last_layer_skip(net) && d_input) used_dzB = true;      // (last_layer_kernel wrote it)
    if (d_input) {
      TRY(add_dz_to_input(c, used_dzB, d_input, ld_din));
      if (xyz_acc) {
        const long long tx = (long long)n * net->geom_dim;
        hipLaunchKernelGGL(acc_cols_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, c.st, c.at<float>(P.dxz_off[1]), 4, d_input,
                           (int)ld_din, net->latent_size, (int)n, net->geom_dim, 1);
        LAUNCH_OK("acc_cols_kernel");
      }
    }
    return 0;
  }
  if (d_input) TRY(add_dz_to_input(c, used_dzB, d_input, ld_din));
  return 0;
}

int dsdf_module_backward(const DsdfNet* net, const float* packed, const float* params, const float* d_sdf, int64_t n,
                         int32_t training, const uint32_t* dropout_key, float* grads, int32_t accumulate, float* d_input,
                         int64_t ld_din, void* ws, size_t ws_bytes, void* stream) {
  return module_backward_impl(net, packed, params, d_sdf, n, training, dropout_key, grads, accumulate, d_input, ld_din, ws, ws_bytes,
                              stream, true);
}

int dsdf_module_input_grad(const DsdfNet* net, const float* packed, const float* params, const float* d_sdf, int64_t n,
                           float* d_input, int64_t ld_din, void* ws, size_t ws_bytes, void* stream) {
  if (n < 0) return fail(DSDF_E_INVALID, "input gradient: %lld rows", (long long)n);
  if (n > 0 && (!d_sdf || !d_input)) return fail(DSDF_E_INVALID, "input gradient: NULL d_sdf or d_input");
  return module_backward_impl(net, packed, params, d_sdf, n, 0, nullptr, nullptr, 0, d_input, ld_din, ws, ws_bytes, stream, false);
}

// Forward-mode tangent of the decoder at the point of the last dsdf_module_forward on this workspace:
//   t_0 = tangent;  t_{l+1} = (in_l-tangent W_l^T) * [a_{l+1} > 0] * mask_scale   (same ReLU / dropout decisions as the primal:
//   the mask is read off the stored activations);  skip layer: in-tangent = [t_l | tangent];  out = tanh' ... tanh' (t_last w_last)
// Layer-by-layer MFMA GEMM launches (gemm.hpp) -- this is the one-extra-pass tool of mesh.py:420, not the training hot path.
int dsdf_module_jvp(const DsdfNet* net, const float* packed, const float* params, const float* tangent, int64_t ld_t,
                    int64_t n, int32_t training, const uint32_t* dropout_key, float* jvp_out, void* ws, size_t ws_bytes, void* stream) {
  Call c;
  const bool lat_drop = net && net->latent_dropout && training && net->latent_size > 0;
  // (FROWS: the layout dsdf_module_forward left its activations in; the launches below use no path)
  const int rc = open_call(c, ENTRY_MODULE_FWD, net, packed, params, ws, ws_bytes, stream, n, [&] {
    if (!tangent || !jvp_out || n < 0 || ld_t < net->in_dim[0]) return fail(DSDF_E_INVALID, "bad tangent/jvp_out/ld_t");
    if (lat_drop && !dropout_key) return fail(DSDF_E_INVALID, "dropout_key is NULL (latent_dropout needs the forward's key)");
    return 0;
  }, FROWS);
  if (rc != 0 || n == 0) return rc;
  const Plan& P = c.P;
  hipStream_t st = c.st;
  const int last = net->n_layers - 1;
  float* t0 = c.at<float>(P.dzA_off);                      // the input tangent in a 16-byte-aligned, zero-padded layout
  HIP_OK(hipMemsetAsync(t0, 0, (size_t)n * P.ldz * 4, st));
  HIP_OK(hipMemsetAsync(c.at<float>(P.dp_off[0]), 0, (size_t)n * P.ld_dp * 4, st));
  HIP_OK(hipMemsetAsync(c.at<float>(P.dp_off[1]), 0, (size_t)n * P.ld_dp * 4, st));
  {
    const long long tot = (long long)n * P.W0;
    hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tangent, (int)ld_t, (const float*)nullptr, 0,
                       t0, (long long)P.ldz, (int)n, P.W0);
    LAUNCH_OK("add2_kernel(tangent)");
  }
  float* t0_layer0 = t0;                                     // latent_dropout: layer 0 sees the tangent of the DROPPED latent,
  if (lat_drop) {                                            // the skip layer the raw one (deep_sdf_decoder.py:79-89)
    t0_layer0 = c.at<float>(P.dzB_off);
    HIP_OK(hipMemcpyAsync(t0_layer0, t0, (size_t)n * P.ldz * 4, hipMemcpyDeviceToDevice, st));
    const long long tot = (long long)n * net->latent_size;
    hipLaunchKernelGGL(latent_drop_bwd_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, t0_layer0, P.ldz, (int)n,
                       net->latent_size, dropout_key[LATENT_DROPOUT_KEY], latent_drop_thr(), 1.0f / (1.0f - LATENT_DROPOUT_P), 0u);
    LAUNCH_OK("latent_drop_bwd_kernel(tangent)");
  }
  auto append = [&](float* in_t, int l) -> int {             // what the forward concatenates to layer l's input, for the tangent
    const bool skip = (net->skip_mask >> l) & 1;
    if (!skip && !net->xyz_in_all) return 0;
    const int w = skip ? P.W0 : net->geom_dim;
    const float* src = skip ? t0 : t0 + net->latent_size;
    const long long tot = (long long)n * w;
    hipLaunchKernelGGL(add2_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, src, P.ldz, (const float*)nullptr, 0,
                       in_t + net->out_dim[l - 1], (long long)P.ld_dp, (int)n, w);
    return 0;
  };
  int cur = 0;
  for (int l = 0; l < last; ++l) {
    float* in_t = l == 0 ? t0_layer0 : c.at<float>(P.dp_off[cur]);
    if (l > 0) { append(in_t, l); LAUNCH_OK("add2_kernel(concat tangent)"); }
    NtArgs a;
    memset(&a, 0, sizeof(a));
    a.A = in_t; a.lda = l == 0 ? P.ldz : P.ld_dp;
    a.B = packed + c.pk.w_off[l]; a.ldb = c.pk.ldw[l];
    a.C = c.at<float>(P.dp_off[l == 0 ? 0 : cur ^ 1]); a.ldc = P.ld_dp;
    a.M = (int)n; a.N = net->out_dim[l]; a.K = net->in_dim[l];
    if (ln_applied(net, l)) {                                // Linear tangent, then LayerNorm + ReLU/dropout in one row pass
      TRY(launch_nt<EPI_PLAIN>(a, st));
      LnJvpArgs j;
      memset(&j, 0, sizeof(j));
      j.t = a.C; j.ldt = a.ldc; j.xhat = c.at<float>(P.lnx_off[l]); j.ldx = P.ld_in[l + 1]; j.rstd = c.at<float>(P.lnr_off[l]);
      j.gamma = params + c.L.ln_w_off[l]; j.act = c.at<float>(P.in_off[l + 1]); j.ldact = P.ld_in[l + 1];
      j.mask_scale = mask_scale_of(net, l, training); j.n = (int)n; j.width = net->out_dim[l];
      hipLaunchKernelGGL(ln_jvp_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, j);
      LAUNCH_OK("ln_jvp_kernel");
    } else {
      a.act = c.at<float>(P.in_off[l + 1]); a.ldact = P.ld_in[l + 1];
      a.mask_cols = net->out_dim[l]; a.mask_scale = mask_scale_of(net, l, training);
      TRY(launch_nt<EPI_BWD>(a, st));
    }
    if (l > 0) cur ^= 1;
  }
  if (last > 0) { append(c.at<float>(P.dp_off[cur]), last); LAUNCH_OK("add2_kernel(concat tangent, last)"); }
  NtArgs a;                                                   // du = t_last . w_last
  memset(&a, 0, sizeof(a));
  a.A = c.at<float>(P.dp_off[cur]); a.lda = P.ld_dp;
  a.B = packed + c.pk.w_off[last]; a.ldb = c.pk.ldw[last];
  a.C = c.at<float>(P.y_off); a.ldc = 1;
  a.M = (int)n; a.N = 1; a.K = net->in_dim[last];
  TRY(launch_nt<EPI_PLAIN>(a, st));
  hipLaunchKernelGGL(jvp_tail_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c.at<float>(P.y_off),
                     c.at<float>(P.u_off), jvp_out, (int)n, net->use_tanh);
  LAUNCH_OK("jvp_tail_kernel");
  return 0;
}

}  // extern "C"

namespace {
// fz != nullptr: sets fz->used when the decoder's Adam update (and the new weight-norm scales) was folded into the finalize pass
int train_fb_impl(const DsdfNet* net, const float* packed, const float* params, float* latent_table, int64_t n_scenes,
                  const DsdfBatch* b, const DsdfLossCfg* cfg, float* grads, float* dlat, float* loss_out, float* sdf_out,
                  int32_t accumulate, void* ws, size_t ws_bytes, void* stream, FuseAdam* fz) {
  Call c;
  TRY(open_call(
      c, ENTRY_TRAIN, net, packed, params, ws, ws_bytes, stream, b ? b->n_points : 0,
      [&] {
        if (!b || !cfg || !latent_table || !grads || !dlat || !loss_out) return fail(DSDF_E_INVALID, "NULL argument");
        if (b->n_points <= 0 || b->n_segments <= 0 || n_scenes <= 0)
          return fail(DSDF_E_INVALID, "empty batch (n_points %lld, n_segments %lld)", (long long)b->n_points, (long long)b->n_segments);
        if (!b->seg_scene || !b->seg_offset || !b->xyz || !b->sdf_gt) return fail(DSDF_E_INVALID, "NULL batch pointer");
        if (b->n_norm <= 0) return fail(DSDF_E_INVALID, "n_norm must be positive");
        if (net->latent_size <= 0) return fail(DSDF_E_INVALID, "training needs latent_size > 0");
        const int phase = cfg->dw_phase, nbk = cfg->dw_buckets;
        if (nbk < 0 || nbk > DSDF_MAX_BUCKETS) return fail(DSDF_E_INVALID, "dw_buckets %d out of range [0, %d]", nbk, DSDF_MAX_BUCKETS);
        if (phase < 0 || (nbk <= 1 ? phase != 0 : phase < 1 || phase > nbk))
          return fail(DSDF_E_INVALID, "dw_phase %d out of range for dw_buckets %d (0 without buckets, 1..K with K >= 2)", phase, nbk);
        return 0;
      },
      [&](const Call& c) {
        // Segment mode: the batch is scenes x samples with every segment a whole number of 64-row workgroups, so a workgroup
        // sees ONE latent vector: its products with the weights are hoisted out of the per-point work (fused.hpp FusedSeg),
        // and the latent gradient / the x0 columns of the weight gradients come from per-workgroup column sums.
        const bool seg = c.path.fused && b->seg_len > 0 && b->seg_len % c.path.frows == 0 && b->seg_len * b->n_segments == c.n &&
                         net->n_layers > 2 &&
                         skip_layer(net) != net->n_layers - 2 &&   // the deepest hidden layer's dP column sums live in the head's partials
                         !last_layer_skip(net) &&
                         net->geom_dim <= FGEO && net->latent_size >= 1 && net->latent_size <= HOIST_MAXL;   // (config 5 too: bf16 rounding
                                                             // is element-wise on the operands, so the latent products still hoist)
        return make_plan(net, c.n, b->n_segments, false, seg, cfg->dw_buckets, c.path.frows, &t_last_plan);
      }));
  c.training = cfg->training; c.keys = cfg->dropout_key; c.row_offset = (uint32_t)b->row_offset;
  const Plan& P = c.P;
  hipStream_t st = c.st;
  const int64_t n = c.n, R = b->n_segments;
  const bool fusedb = c.path.fused, merged = c.path.merged, segsum = P.segmode != 0;
  const int phase = cfg->dw_phase, Lc = net->latent_size;
  if (phase != 0 && (!fusedb || cfg->frozen_decoder || accumulate || fz != nullptr))
    return fail(DSDF_E_INVALID, "dw_phase needs the fused kernels (dsdf_dw_phase_supported), a trainable decoder, accumulate = 0 and the two-call path");
  if (phase >= 2) {   // only the weight gradients of bucket phase - 1, from what the phase-1 call left in the workspace
    FusedSeg seg0;
    memset(&seg0, 0, sizeof(seg0));
    const FusedBwdHead h0 = make_head(c, HEAD_TRAIN);
    const SegBwd sb0{&seg0, b->seg_scene, latent_table, (int)R, nullptr, nullptr, nullptr};
    bool used = false;
    return run_backward_fused(c, GradSink{grads, 0, nullptr}, segsum ? 0 : Lc, &used, true, h0, segsum ? &sb0 : nullptr, nullptr, phase);
  }

  if (!segsum && (cfg->code_bound > 0.f || !accumulate)) {   // max-norm renorm of the looked-up rows + zero of the dense latent gradient
    // (segment mode: both are part of the hoist launch -- seg_hoist_kernel)
    const long long nzero = accumulate ? 0 : (long long)n_scenes * Lc;
    long long blocks = (R + 3) / 4, zb = (nzero + 4095) / 4096;
    if (zb > 2048) zb = 2048;
    if (zb > blocks) blocks = zb;
    hipLaunchKernelGGL(latent_renorm_kernel, dim3((unsigned)blocks), dim3(256), 0, st, latent_table, Lc, b->seg_scene, (int)R,
                       cfg->code_bound > 0.f ? cfg->code_bound : 0.f, accumulate ? nullptr : dlat, nzero);
    LAUNCH_OK("latent_renorm_kernel");
  }
  FusedSeg seg;
  memset(&seg, 0, sizeof(seg));
  FusedFwdArgs fwd_args;                                   // merged: forward + backward go out as ONE launch below
  if (segsum) {
    const HoistRenorm hr{cfg->code_bound > 0.f ? cfg->code_bound : 0.f, dlat, accumulate ? 0 : (long long)n_scenes * Lc};
    TRY(run_hoist(c, latent_table, b, &seg, &hr));
    TRY(run_fused_forward(c, true, nullptr, nullptr, &seg, merged ? &fwd_args : nullptr));
  } else {
    TRY(run_gather(c, latent_table, b, nullptr, 0));
    if (fusedb) TRY(run_fused_forward(c, true, nullptr, nullptr, nullptr, merged ? &fwd_args : nullptr));
    else TRY(run_hidden_forward(c));
  }

  if (!fusedb) {
    LastArgs a = last_args(c, true);
    a.y_out = sdf_out; a.gt = b->sdf_gt; a.delta = cfg->clamp_dist; a.inv_n = 1.0f / (float)b->n_norm;
    if (last_layer_skip(net)) { a.dz = c.at<float>(P.dzB_off); a.ldz = P.ldz; a.dz_cols = Lc; }
    TRY(launch_last<LAST_TRAIN>(a, P.last_blocks, st));
  }

  bool used_dzB = false;
  const bool want_dw = cfg->frozen_decoder == 0;
  ScatterArgs sc;   // dense latent gradient + regulariser + loss (block 0); launched below unless it rode on the finalize launch
  memset(&sc, 0, sizeof(sc));
  sc.segpart = c.at<float>(P.segpart_off); sc.segnorm = c.at<float>(P.segnorm_off);
  sc.seg_scene = b->seg_scene; sc.seg_offset = b->seg_offset;
  sc.R = (int)R; sc.L = Lc; sc.table = latent_table; sc.dlat = dlat;
  sc.zr = segsum ? c.at<float>(P.zr_off) : nullptr;
  sc.creg = cfg->reg_coef / (float)b->n_norm;
  sc.part_loss = c.at<float>(P.partloss_off); sc.n_part = fusedb ? P.nwg : P.last_blocks;
  sc.loss_scale = 1.0f / (float)b->n_norm; sc.loss_out = loss_out; sc.accumulate = accumulate;
  bool scatter_done = false;
  if (fusedb) {
    FusedBwdHead h = make_head(c, HEAD_TRAIN);
    h.gt = b->sdf_gt; h.delta = cfg->clamp_dist; h.inv_n = 1.0f / (float)b->n_norm; h.y_out = sdf_out;
    const FuseAdam* use = (fz != nullptr && want_dw && !accumulate) ? fz : nullptr;
    const SegBwd sb{&seg, b->seg_scene, latent_table, (int)R, &sc, &scatter_done, sc.zr};
    TRY(run_backward_fused(c, GradSink{grads, accumulate, use}, segsum ? 0 : Lc, &used_dzB, want_dw, h, segsum ? &sb : nullptr,
                           merged ? &fwd_args : nullptr, phase));
    if (use != nullptr) fz->used = true;
  } else {
    TRY(run_backward(c, GradSink{grads, accumulate, nullptr}, Lc, &used_dzB, want_dw));
    if (last_layer_skip(net)) used_dzB = true;                 // (last_layer_kernel wrote it)
  }

  SegArgs s;
  memset(&s, 0, sizeof(s));
  s.dzA = c.at<float>(P.dzA_off); s.dzB = used_dzB ? c.at<float>(P.dzB_off) : nullptr; s.ldz = P.ldz;
  s.seg_scene = b->seg_scene; s.seg_offset = b->seg_offset; s.R = (int)R; s.L = Lc; s.table = latent_table;
  s.segpart = c.at<float>(P.segpart_off); s.segnorm = c.at<float>(P.segnorm_off);
  if (!segsum) {   // (segment mode: per-segment latent gradients came out of post_bwd_kernel)
    // few long segments: cut their rows into slices until the launch has blocks for the chip (the scatter adds the slices)
    int nsl = 1;
    const long long blocks = (long long)R * ((Lc + 63) / 64);
    while (nsl < LAT_SLICES_MAX && blocks * nsl * 2 <= chip_waves() / 4 && n / (R * (int64_t)nsl * 2) >= 128) nsl *= 2;
    s.nslice = nsl; s.slice_stride = (long long)R * Lc;
    sc.nslice = nsl; sc.slice_stride = s.slice_stride;
    hipLaunchKernelGGL(seg_reduce_kernel, dim3((unsigned)R, (Lc + 63) / 64, (unsigned)nsl), dim3(256), 0, st, s);
    LAUNCH_OK("seg_reduce_kernel");
  }
  if (!scatter_done) {
    hipLaunchKernelGGL(seg_scatter_kernel, dim3((unsigned)R), dim3(256), 0, st, sc);   // + the loss (block 0)
    LAUNCH_OK("seg_scatter_kernel");
  }
  return 0;
}
}  // namespace

extern "C" {

int dsdf_train_forward_backward(const DsdfNet* net, const float* packed, const float* params, float* latent_table,
                                int64_t n_scenes, const DsdfBatch* b, const DsdfLossCfg* cfg, float* grads, float* dlat,
                                float* loss_out, float* sdf_out, int32_t accumulate, void* ws, size_t ws_bytes,
                                void* stream) {
  return train_fb_impl(net, packed, params, latent_table, n_scenes, b, cfg, grads, dlat, loss_out, sdf_out, accumulate, ws,
                       ws_bytes, stream, nullptr);
}

int dsdf_grad_norm(const float* grads, int64_t n, float max_norm, float* norm_out, float* coef_out, void* ws,
                   size_t ws_bytes, void* stream) {
  if (!grads || !norm_out || !coef_out || !ws || n <= 0) return fail(DSDF_E_INVALID, "bad arguments");
  int blocks = (int)((n + 4095) / 4096);
  if (blocks > 1024) blocks = 1024;
  WsCarver c(&t_last_plan, 1);
  c.take("gn_partials", -1, (size_t)blocks * 4);
  if (ws_bytes < c.finish(c.o)) return fail(DSDF_E_WORKSPACE, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(256), 0, st, grads, (long long)n, (float*)ws);
  LAUNCH_OK("sumsq_partial_kernel");
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, blocks, max_norm, norm_out, coef_out);
  LAUNCH_OK("clip_coef_kernel");
  return 0;
}

static int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr, const DsdfAdamCfg* c,
                       const float* gscale, hipStream_t st) {
  if (n <= 0) return 0;
  const double bc1 = 1.0 - pow((double)c->beta1, (double)c->step);
  const double bc2 = 1.0 - pow((double)c->beta2, (double)c->step);
  const float step_size = (float)((double)lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, st, p, g, m, v, (long long)n, 1.0f - c->beta1, c->beta2,
                     1.0f - c->beta2, step_size, bc2_sqrt, c->eps, gscale);
  LAUNCH_OK("adam_kernel");
  return 0;
}

int dsdf_adam_step(const DsdfNet* net, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   float* latent_table, const float* dlat, float* lat_exp_avg, float* lat_exp_avg_sq,
                   int64_t n_latent_floats, const DsdfAdamCfg* cfg, float* packed, void* stream) {
  TRY(validate(net));
  if (!params || !grads || !exp_avg || !exp_avg_sq || !cfg || !packed) return fail(DSDF_E_INVALID, "NULL argument");
  if (cfg->step < 1) return fail(DSDF_E_INVALID, "Adam step must be >= 1");
  hipStream_t st = (hipStream_t)stream;
  DsdfParamLayout L;
  param_layout(net, &L);
  {   // decoder: Adam per (layer, row) + the row's new weight-norm scale in one pass
    const Packed pk = packed_layout(net);
    AdamRowsArgs a;
    memset(&a, 0, sizeof(a));
    a.nl = net->n_layers; a.p = params; a.g = grads; a.m = exp_avg; a.s = exp_avg_sq; a.scale = packed + pk.scale_off;
    const double bc1 = 1.0 - pow((double)cfg->beta1, (double)cfg->step), bc2 = 1.0 - pow((double)cfg->beta2, (double)cfg->step);
    a.omb1 = 1.0f - cfg->beta1; a.b2 = cfg->beta2; a.omb2 = 1.0f - cfg->beta2;
    a.step_size = (float)((double)cfg->lr_decoder / bc1); a.bc2_sqrt = (float)sqrt(bc2); a.eps = cfg->eps; a.gscale = cfg->grad_scale;
    int rows = 0;
    for (int l = 0; l < net->n_layers; ++l) {
      a.ly[l] = AdamRowsLayer{L.v_off[l], L.g_off[l], L.bias_off[l], net->out_dim[l], net->in_dim[l], rows};
      rows += net->out_dim[l];
    }
    a.total_rows = rows;
    hipLaunchKernelGGL(adam_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, a);
    LAUNCH_OK("adam_rows_kernel");
    for (int l = 0; l < net->n_layers; ++l)     // LayerNorm variant: bn{l}.weight | bn{l}.bias are adjacent in the arena
      if (L.ln_w_off[l] >= 0)
        TRY(adam_launch(params + L.ln_w_off[l], grads + L.ln_w_off[l], exp_avg + L.ln_w_off[l], exp_avg_sq + L.ln_w_off[l],
                        2 * (int64_t)net->out_dim[l], cfg->lr_decoder, cfg, cfg->grad_scale, st));
  }
  if (n_latent_floats > 0) {
    if (!latent_table || !dlat || !lat_exp_avg || !lat_exp_avg_sq) return fail(DSDF_E_INVALID, "NULL latent argument");
    const AdamRide ride = adam_ride(latent_table, dlat, lat_exp_avg, lat_exp_avg_sq, n_latent_floats, cfg->lr_latent, cfg);
    return materialize(net, params, packed, st, true, &ride);
  }
  return materialize(net, params, packed, st, true);
}

int dsdf_train_step(const DsdfNet* net, float* packed, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                    float* latent_table, int64_t n_scenes, float* dlat, float* lat_exp_avg, float* lat_exp_avg_sq,
                    const DsdfBatch* b, const DsdfLossCfg* cfg, const DsdfAdamCfg* adam, float* loss_out, float* sdf_out,
                    void* ws, size_t ws_bytes, void* stream) {
  if (!adam || !exp_avg || !exp_avg_sq || !lat_exp_avg || !lat_exp_avg_sq) return fail(DSDF_E_INVALID, "NULL argument");
  if (adam->step < 1) return fail(DSDF_E_INVALID, "Adam step must be >= 1");
  FuseAdam fz{adam, params, exp_avg, exp_avg_sq, packed, false};
  const bool can_fuse = adam->grad_scale == nullptr && cfg && !cfg->frozen_decoder;
  TRY(train_fb_impl(net, packed, params, latent_table, n_scenes, b, cfg, grads, dlat, loss_out, sdf_out, 0, ws, ws_bytes, stream,
                    can_fuse ? &fz : nullptr));
  const int64_t nlat = n_scenes * net->latent_size;
  if (!fz.used)
    return dsdf_adam_step(net, params, grads, exp_avg, exp_avg_sq, latent_table, dlat, lat_exp_avg, lat_exp_avg_sq, nlat, adam,
                          packed, stream);
  hipStream_t st = (hipStream_t)stream;
  const AdamRide ride = adam_ride(latent_table, dlat, lat_exp_avg, lat_exp_avg_sq, nlat, adam->lr_latent, adam);
  return materialize(net, params, packed, st, true, &ride);   // latent Adam + W / W^T / fragment copies in one launch
}

int dsdf_adam_latent_only(float* latent, const float* dlat, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const DsdfAdamCfg* cfg, void* stream) {
  if (!latent || !dlat || !exp_avg || !exp_avg_sq || !cfg || n <= 0) return fail(DSDF_E_INVALID, "bad arguments");
  if (cfg->step < 1) return fail(DSDF_E_INVALID, "Adam step must be >= 1");
  return adam_launch(latent, dlat, exp_avg, exp_avg_sq, n, cfg->lr_latent, cfg, nullptr, (hipStream_t)stream);
}

int dsdf_adam_latent_sched(float* latent, const float* dlat, float* exp_avg, float* exp_avg_sq, int64_t n, const float* sched,
                           int64_t n_steps, int64_t* step_counter, float beta1, float beta2, float eps, float l2_coef, void* stream) {
  if (!latent || !dlat || !exp_avg || !exp_avg_sq || !sched || !step_counter || n <= 0 || n_steps <= 0)
    return fail(DSDF_E_INVALID, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_sched_kernel, dim3(blocks), dim3(256), 0, st, latent, dlat, exp_avg, exp_avg_sq, (long long)n, sched,
                     (long long)n_steps, (const long long*)step_counter, 1.0f - beta1, beta2, 1.0f - beta2, eps, l2_coef);
  LAUNCH_OK("adam_sched_kernel");
  hipLaunchKernelGGL(counter_inc_kernel, dim3(1), dim3(1), 0, st, (long long*)step_counter);
  LAUNCH_OK("counter_inc_kernel");
  return 0;
}

static int sample_launch(const float* data, int32_t geom_dim, const int64_t* pos_start, const int64_t* n_pos, const int64_t* neg_start,
                         const int64_t* n_neg, const int64_t* scene_ids, int64_t n_batch_scenes, int64_t subsample, uint64_t key,
                         uint64_t key_step, const int64_t* counter, float* xyz_out, float* sdf_out, void* stream) {
  if (!data || !pos_start || !n_pos || !neg_start || !n_neg || !scene_ids || !xyz_out || !sdf_out)
    return fail(DSDF_E_INVALID, "NULL argument");
  if (geom_dim < 1 || geom_dim > 16) return fail(DSDF_E_INVALID, "geom_dim %d out of range", geom_dim);
  const int64_t S = 2 * (subsample / 2);
  if (n_batch_scenes <= 0 || S <= 0 || n_batch_scenes * S > (1ll << 31) - 1) return fail(DSDF_E_INVALID, "bad batch shape");
  SampleArgs a;
  memset(&a, 0, sizeof(a));
  a.data = data; a.row_floats = geom_dim + 1; a.G = geom_dim;
  a.pos_start = pos_start; a.n_pos = n_pos; a.neg_start = neg_start; a.n_neg = n_neg;
  a.scene_ids = scene_ids; a.B = (int)n_batch_scenes; a.S = (int)S; a.key = key; a.xyz = xyz_out; a.sdf = sdf_out;
  a.counter = (const long long*)counter; a.key_step = key_step;
  const long long tot = n_batch_scenes * S;
  hipLaunchKernelGGL(sample_batch_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  LAUNCH_OK("sample_batch_kernel");
  return 0;
}

int dsdf_sample_batch(const float* data, int32_t geom_dim, const int64_t* pos_start, const int64_t* n_pos,
                      const int64_t* neg_start, const int64_t* n_neg, const int64_t* scene_ids, int64_t n_batch_scenes,
                      int64_t subsample, uint64_t key, float* xyz_out, float* sdf_out, void* stream) {
  return sample_launch(data, geom_dim, pos_start, n_pos, neg_start, n_neg, scene_ids, n_batch_scenes, subsample, key, 0, nullptr, xyz_out,
                       sdf_out, stream);
}

int dsdf_sample_batch_seq(const float* data, int32_t geom_dim, const int64_t* pos_start, const int64_t* n_pos,
                          const int64_t* neg_start, const int64_t* n_neg, const int64_t* scene_ids, int64_t n_batch_scenes,
                          int64_t subsample, uint64_t key0, uint64_t key_step, const int64_t* counter, float* xyz_out, float* sdf_out,
                          void* stream) {
  if (!counter) return fail(DSDF_E_INVALID, "counter is NULL");
  return sample_launch(data, geom_dim, pos_start, n_pos, neg_start, n_neg, scene_ids, n_batch_scenes, subsample, key0, key_step, counter,
                       xyz_out, sdf_out, stream);
}

int dsdf_profile_enable(int32_t on) {
  g_prof.on = on != 0;
  g_prof.used = 0;
  for (int c = 0; c < Prof::NCLS; ++c) g_prof.flops[c] = 0;
  return 0;
}

int dsdf_profile_read(DsdfProfile* out) {
  if (!out) return fail(DSDF_E_INVALID, "out is NULL");
  memset(out, 0, sizeof(*out));
  Prof& P = g_prof;
  for (int i = 0; i < P.used; ++i) {
    HIP_OK(hipEventSynchronize(P.ev[i][1]));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, P.ev[i][0], P.ev[i][1]));
    out->ms[P.cls[i]] += ms;
    out->count[P.cls[i]] += 1;
  }
  for (int c = 0; c < Prof::NCLS; ++c) out->flops[c] = P.flops[c];
  out->dropped = P.used >= Prof::POOL;
  P.used = 0;
  for (int c = 0; c < Prof::NCLS; ++c) P.flops[c] = 0;
  return 0;
}

int dsdf_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N,
                 int64_t K, const float* bias, void* stream) {
  if (!A || !B || !C) return fail(DSDF_E_INVALID, "NULL operand");
  NtArgs a;
  memset(&a, 0, sizeof(a));
  a.A = A; a.B = B; a.C = C; a.lda = (int)lda; a.ldb = (int)ldb; a.ldc = (int)ldc; a.M = (int)M; a.N = (int)N; a.K = (int)K;
  a.bias = bias;
  return launch_nt<EPI_PLAIN>(a, (hipStream_t)stream);
}

int dsdf_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int64_t N,
                 int64_t K, void* ws, size_t ws_bytes, void* stream) {
  if (!A || !B || !C || !ws) return fail(DSDF_E_INVALID, "NULL operand");
  int ns = (int)((K + 255) / 256);
  if (ns > NSPLIT_MAX) ns = NSPLIT_MAX;
  if (ns < 1) ns = 1;
  const int kchunk = (int)rup((K + ns - 1) / ns, BK);
  const int nsplit = (int)((K + kchunk - 1) / kchunk);
  const long long slab = rup(M * ldc, 64);
  if (ws_bytes < (size_t)nsplit * slab * 4) return fail(DSDF_E_WORKSPACE, "gemm_tn needs %lld bytes of workspace", (long long)nsplit * slab * 4);
  TnArgs t;
  memset(&t, 0, sizeof(t));
  t.A = A; t.B = B; t.C = (float*)ws; t.lda = (int)lda; t.ldb = (int)ldb; t.ldc = (int)ldc; t.M = (int)M; t.N = (int)N;
  t.K = (int)K; t.kchunk = kchunk; t.slab = slab;
  hipStream_t st = (hipStream_t)stream;
  TRY(launch_tn(t, nsplit, st));
  // plain fixed-order slab sum (no weight norm): reuse the finalize kernel with g == NULL and no bias partials
  FinArgs f;
  memset(&f, 0, sizeof(f));
  if (N > 2048 || ldc != N) return fail(DSDF_E_INVALID, "gemm_tn test entry needs ldc == N <= 2048");
  f.slabs = t.C; f.nsplit = nsplit; f.slab = slab; f.ldc = (int)ldc; f.colsum = nullptr; f.npart = 0; f.ldcs = 0;
  WsCarver c(&t_last_plan, 1);
  c.take("tn_slabs", -1, (size_t)nsplit * slab * 4);
  f.dv = C; f.db = (float*)((char*)ws + c.take("tn_db", -1, (size_t)M * 4));   // scratch row of M floats behind the slabs
  if (ws_bytes < c.finish(c.o)) return fail(DSDF_E_WORKSPACE, "gemm_tn workspace too small");
  f.out = (int)M; f.in = (int)N;
  hipLaunchKernelGGL(finalize_layer_kernel, dim3((unsigned)M), dim3(256), 0, st, f);
  LAUNCH_OK("finalize_layer_kernel(test)");
  return 0;
}

int dsdf_dropout_mask(uint32_t key, float p, int64_t rows, int64_t cols, int64_t row_offset, uint8_t* out, void* stream) {
  if (!out || rows <= 0 || cols <= 0) return fail(DSDF_E_INVALID, "bad arguments");
  long thr = lround((double)p * 65536.0);
  if (thr > 65535) thr = 65535;
  const long long tot = rows * cols;
  hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, key,
                     (uint32_t)thr, (int)rows, (int)cols, (uint32_t)row_offset, out);
  LAUNCH_OK("dropout_mask_kernel");
  return 0;
}

// ---- marching cubes (mcubes.hpp) ----------------------------------------------------------------------
namespace {
struct McPlan {
  int64_t npts, nblocks;
  size_t mask, cas, vbase, bv, bf, ov, of, total;
};

// The grid every mesher and the sparse grid accept: 2 .. MC_MAX_DIM points per axis.
int grid_dims_ok(const char* what, int32_t nx, int32_t ny, int32_t nz) {
  if (nx < 2 || ny < 2 || nz < 2 || nx > MC_MAX_DIM || ny > MC_MAX_DIM || nz > MC_MAX_DIM)
    return fail(DSDF_E_INVALID, "%s: grid %d x %d x %d outside [2, %d] per axis", what, nx, ny, nz, MC_MAX_DIM);
  return 0;
}

int mc_plan(int32_t nx, int32_t ny, int32_t nz, McPlan* P, WsTable* rec = nullptr) {
  TRY(grid_dims_ok("marching cubes", nx, ny, nz));
  P->npts = (int64_t)nx * ny * nz;
  P->nblocks = (P->npts + MC_BLOCK - 1) / MC_BLOCK;
  WsCarver c(rec);
  P->mask = c.take("mc_mask", -1, (size_t)P->npts);
  P->cas = c.take("mc_cas", -1, (size_t)P->npts);
  P->vbase = c.take("mc_vbase", -1, (size_t)P->npts * 4);
  P->bv = c.take("mc_bv", -1, (size_t)P->nblocks * 4);
  P->bf = c.take("mc_bf", -1, (size_t)P->nblocks * 4);
  P->ov = c.take("mc_ov", -1, (size_t)(P->nblocks + 1) * 8);
  P->of = c.take("mc_of", -1, (size_t)(P->nblocks + 1) * 8);
  P->total = c.finish(c.o);
  return 0;
}

void mc_bind(const McPlan& P, void* ws, McWs* w) {
  char* b = (char*)ws;
  w->mask = (uint8_t*)(b + P.mask); w->cas = (uint8_t*)(b + P.cas); w->vbase = (int32_t*)(b + P.vbase);
  w->bv = (int32_t*)(b + P.bv); w->bf = (int32_t*)(b + P.bf); w->ov = (int64_t*)(b + P.ov); w->of = (int64_t*)(b + P.of);
  w->nblocks = P.nblocks;
}

int mc_setup(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, void* ws, size_t ws_bytes, McGrid* g,
             McWs* w, McPlan* P) {
  TRY(mc_plan(nx, ny, nz, P, &t_last_plan));
  if (!sdf || !ws) return fail(DSDF_E_INVALID, "marching cubes: NULL sdf or workspace");
  if (ws_bytes < P->total) return fail(DSDF_E_WORKSPACE, "marching cubes: workspace %zu < %zu bytes", ws_bytes, P->total);
  g->sdf = sdf; g->nx = nx; g->ny = ny; g->nz = nz; g->level = level; g->npts = P->npts;
  mc_bind(*P, ws, w);
  return 0;
}
}  // namespace

int dsdf_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes) {
  McPlan P;
  TRY(mc_plan(nx, ny, nz, &P, &t_last_plan));
  if (!bytes) return fail(DSDF_E_INVALID, "NULL bytes");
  *bytes = P.total;
  return 0;
}

int dsdf_mc_count(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* totals, void* ws, size_t ws_bytes,
                  void* stream) {
  McGrid g; McWs w; McPlan P;
  TRY(mc_setup(sdf, nx, ny, nz, level, ws, ws_bytes, &g, &w, &P));
  if (!totals) return fail(DSDF_E_INVALID, "marching cubes: NULL totals");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_classify_kernel, dim3((unsigned)P.nblocks), dim3(MC_BLOCK), 0, st, g, w);
  LAUNCH_OK("mc_classify_kernel");
  const OffsetScan<2> scan = {{w.bv, w.bf}, {w.ov, w.of}, w.nblocks, totals};
  hipLaunchKernelGGL(offset_scan_kernel<2>, dim3(1), dim3(MC_SCAN_THREADS), 0, st, scan);
  LAUNCH_OK("offset_scan_kernel<2>");
  return 0;
}

int dsdf_mc_emit(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing, const float* origin,
                 int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, void* ws, size_t ws_bytes, void* stream) {
  McGrid g; McWs w; McPlan P;
  TRY(mc_setup(sdf, nx, ny, nz, level, ws, ws_bytes, &g, &w, &P));
  if (n_verts < 0 || n_faces < 0 || n_verts > INT32_MAX || n_faces > INT32_MAX)
    return fail(DSDF_E_INVALID, "marching cubes: %lld vertices / %lld faces (int32 indices hold at most %d)", (long long)n_verts,
                (long long)n_faces, INT32_MAX);
  if (!spacing || !origin) return fail(DSDF_E_INVALID, "marching cubes: NULL spacing or origin");
  if ((n_verts > 0 && !verts) || (n_faces > 0 && !faces)) return fail(DSDF_E_INVALID, "marching cubes: NULL verts or faces");
  if (n_verts == 0 && n_faces == 0) return 0;
  McOut o;
  for (int a = 0; a < 3; ++a) { o.spacing[a] = spacing[a]; o.origin[a] = origin[a]; }
  o.verts = verts; o.faces = faces; o.nv = n_verts; o.nf = n_faces;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mc_vertex_kernel, dim3((unsigned)P.nblocks), dim3(MC_BLOCK), 0, st, g, w, o);
  LAUNCH_OK("mc_vertex_kernel");
  if (n_faces > 0) {
    hipLaunchKernelGGL(mc_face_kernel, dim3((unsigned)P.nblocks), dim3(MC_BLOCK), 0, st, g, w, o);
    LAUNCH_OK("mc_face_kernel");
  }
  return 0;
}

int dsdf_mc_edges(int32_t nx, int32_t ny, int32_t nz, int64_t n_verts, int64_t* edge_point, int32_t* edge_axis, void* ws,
                  size_t ws_bytes, void* stream) {
  McPlan P;
  TRY(mc_plan(nx, ny, nz, &P, &t_last_plan));
  if (n_verts < 0 || n_verts > INT32_MAX)
    return fail(DSDF_E_INVALID, "marching cubes edges: %lld vertices (0 .. %d)", (long long)n_verts, INT32_MAX);
  if (!ws) return fail(DSDF_E_INVALID, "marching cubes edges: NULL workspace");
  if (ws_bytes < P.total) return fail(DSDF_E_WORKSPACE, "marching cubes edges: workspace %zu < %zu bytes", ws_bytes, P.total);
  if (n_verts > 0 && (!edge_point || !edge_axis)) return fail(DSDF_E_INVALID, "marching cubes edges: NULL edge_point or edge_axis");
  if (n_verts == 0) return 0;
  McWs w;
  mc_bind(P, ws, &w);
  hipLaunchKernelGGL(mc_edge_kernel, dim3((unsigned)P.nblocks), dim3(MC_BLOCK), 0, (hipStream_t)stream, P.npts, w, n_verts, edge_point,
                     edge_axis);
  LAUNCH_OK("mc_edge_kernel");
  return 0;
}

int dsdf_mc_case_table(int8_t* table, size_t table_bytes, int32_t* width) {
  if (width) *width = MC_TABLE_W;
  if (!table) return width ? 0 : fail(DSDF_E_INVALID, "NULL table and width");
  if (table_bytes < sizeof(mc_tri_h)) return fail(DSDF_E_INVALID, "case table needs %zu bytes", sizeof(mc_tri_h));
  memcpy(table, mc_tri_h, sizeof(mc_tri_h));
  return 0;
}

// ---- mesh SDF (meshsdf.hpp) ----------------------------------------------------------------------------
namespace {
struct MsdfPlan {
  int32_t n_splits, chunk;
  int64_t qblocks;
  size_t tri, ws;
};

int msdf_plan(int64_t nf, int64_t nq, MsdfPlan* P, WsTable* rec = nullptr) {
  if (nf <= 0) return fail(DSDF_E_INVALID, "mesh sdf: %lld faces (need at least one)", (long long)nf);
  if (nq < 0) return fail(DSDF_E_INVALID, "mesh sdf: %lld queries", (long long)nq);
  if (nf > INT32_MAX || nq > INT32_MAX)
    return fail(DSDF_E_INVALID, "mesh sdf: %lld faces / %lld queries (the kernels index in int32: at most %d)", (long long)nf,
                (long long)nq, INT32_MAX);
  P->qblocks = (nq + MSDF_BLOCK - 1) / MSDF_BLOCK;
  int64_t ns = 1;
  if (P->qblocks > 0 && P->qblocks < MSDF_TARGET_WG) {
    ns = (MSDF_TARGET_WG + P->qblocks - 1) / P->qblocks;
    ns = std::min<int64_t>(ns, std::min<int64_t>(nf / MSDF_MIN_SPLIT_FACES, MSDF_MAX_SPLITS));
    ns = std::max<int64_t>(ns, 1);
  }
  P->n_splits = (int32_t)ns;
  P->chunk = (int32_t)((nf + ns - 1) / ns);
  P->tri = (size_t)nf * sizeof(MsdfTri);
  WsCarver c(rec, 1);
  c.take("msdf_partials", -1, (size_t)ns * (size_t)nq * 12);          // d2, face, winding per (split, query): one block
  P->ws = c.finish(c.o);
  return 0;
}
}  // namespace

int dsdf_msdf_plan(int64_t n_faces, int64_t n_queries, size_t* tri_bytes, size_t* ws_bytes, int32_t* n_splits) {
  MsdfPlan P;
  TRY(msdf_plan(n_faces, n_queries, &P, &t_last_plan));
  if (!tri_bytes && !ws_bytes && !n_splits) return fail(DSDF_E_INVALID, "mesh sdf plan: every output is NULL");
  if (tri_bytes) *tri_bytes = P.tri;
  if (ws_bytes) *ws_bytes = P.ws;
  if (n_splits) *n_splits = P.n_splits;
  return 0;
}

int dsdf_msdf_prepare(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* tri, size_t tri_bytes,
                      void* stream) {
  MsdfPlan P;
  TRY(msdf_plan(n_faces, 0, &P));
  if (n_verts <= 0 || n_verts > INT32_MAX)
    return fail(DSDF_E_INVALID, "mesh sdf: %lld vertices (need 1 .. %d)", (long long)n_verts, INT32_MAX);
  if (!verts || !faces || !tri) return fail(DSDF_E_INVALID, "mesh sdf prepare: NULL verts, faces or record buffer");
  if (tri_bytes < P.tri) return fail(DSDF_E_WORKSPACE, "mesh sdf prepare: record buffer %zu < %zu bytes", tri_bytes, P.tri);
  if (((uintptr_t)tri & 15) != 0) return fail(DSDF_E_INVALID, "mesh sdf prepare: record buffer not 16-byte aligned");
  const unsigned blocks = (unsigned)((n_faces + MSDF_PREP_BLOCK - 1) / MSDF_PREP_BLOCK);
  hipLaunchKernelGGL(msdf_prepare_kernel, dim3(blocks), dim3(MSDF_PREP_BLOCK), 0, (hipStream_t)stream, verts, (int)n_verts,
                     faces, (int)n_faces, (MsdfTri*)tri);
  LAUNCH_OK("msdf_prepare_kernel");
  return 0;
}

int dsdf_msdf_query(const void* tri, int64_t n_faces, const float* queries, int64_t n_queries, float* sdf, float* sqr_dist,
                    int32_t* face, float* closest, float* winding, int32_t flip_sign, void* ws, size_t ws_bytes, void* stream) {
  MsdfPlan P;
  TRY(msdf_plan(n_faces, n_queries, &P, &t_last_plan));
  if (!sdf && !sqr_dist && !face && !closest && !winding) return fail(DSDF_E_INVALID, "mesh sdf query: every output is NULL");
  if (n_queries == 0) return 0;
  if (!tri || !queries) return fail(DSDF_E_INVALID, "mesh sdf query: NULL record buffer or queries");
  if (((uintptr_t)tri & 15) != 0) return fail(DSDF_E_INVALID, "mesh sdf query: record buffer not 16-byte aligned");
  if (!ws) return fail(DSDF_E_INVALID, "mesh sdf query: NULL workspace");
  if (ws_bytes < P.ws) return fail(DSDF_E_WORKSPACE, "mesh sdf query: workspace %zu < %zu bytes", ws_bytes, P.ws);
  const bool dist = sdf || sqr_dist || face || closest, wind = sdf || winding;
  const size_t slab = (size_t)P.n_splits * (size_t)n_queries;
  MsdfPartial part;
  part.d2 = (float*)ws;
  part.face = (int32_t*)((char*)ws + slab * 4);
  part.wind = (float*)((char*)ws + slab * 8);
  const MsdfTri* t = (const MsdfTri*)tri;
  const int nf = (int)n_faces, nq = (int)n_queries;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)P.qblocks, (unsigned)P.n_splits);
  if (dist && wind)
    hipLaunchKernelGGL((msdf_query_kernel<true, true>), grid, dim3(MSDF_BLOCK), 0, st, t, nf, P.chunk, queries, nq, part);
  else if (dist)
    hipLaunchKernelGGL((msdf_query_kernel<true, false>), grid, dim3(MSDF_BLOCK), 0, st, t, nf, P.chunk, queries, nq, part);
  else
    hipLaunchKernelGGL((msdf_query_kernel<false, true>), grid, dim3(MSDF_BLOCK), 0, st, t, nf, P.chunk, queries, nq, part);
  LAUNCH_OK("msdf_query_kernel");
  MsdfOut o;
  o.sdf = sdf; o.d2 = sqr_dist; o.face = face; o.closest = closest; o.winding = winding; o.flip = flip_sign != 0;
  hipLaunchKernelGGL(msdf_combine_kernel, dim3((unsigned)P.qblocks), dim3(MSDF_BLOCK), 0, st, t, queries, nq, P.n_splits,
                     (int)dist, (int)wind, part, o);
  LAUNCH_OK("msdf_combine_kernel");
  return 0;
}

// ---- point sets (pointset.hpp) -------------------------------------------------------------------------
namespace {
struct NnPlan {
  int32_t n_splits, chunk;
  int64_t tiles;
  size_t ws;
};

int nn_plan(int64_t nq, int64_t nr, NnPlan* P, WsTable* rec = nullptr) {
  if (nr <= 0) return fail(DSDF_E_INVALID, "nearest neighbour: %lld reference points (need at least one)", (long long)nr);
  if (nq < 0) return fail(DSDF_E_INVALID, "nearest neighbour: %lld queries", (long long)nq);
  if (nr > INT32_MAX || nq > INT32_MAX)
    return fail(DSDF_E_INVALID, "nearest neighbour: %lld queries / %lld reference points (the kernels index in int32: at most %d)",
                (long long)nq, (long long)nr, INT32_MAX);
  P->tiles = (nq + NN_TILE - 1) / NN_TILE;
  int64_t ns = 1;
  if (P->tiles > 0 && P->tiles < NN_TARGET_WG) {
    ns = (NN_TARGET_WG + P->tiles - 1) / P->tiles;
    ns = std::min<int64_t>(ns, std::min<int64_t>(nr / NN_MIN_SPLIT_REFS, NN_MAX_SPLITS));
    ns = std::max<int64_t>(ns, 1);
  }
  P->n_splits = (int32_t)ns;
  P->chunk = (int32_t)((nr + ns - 1) / ns);
  const size_t part = ns > 1 ? (size_t)ns * (size_t)nq * 8 : 0;          // d2 and index per (split, query); one split writes the outputs
  WsCarver c(rec, 1);
  if (part) c.take("nn_partials", -1, part);
  P->ws = c.finish(c.o);
  return 0;
}

struct SurfPlan {
  int64_t tiles;
  size_t tile_off, area_off, bytes;
};

int surf_plan(int64_t nf, SurfPlan* P) {
  if (nf <= 0) return fail(DSDF_E_INVALID, "surface sampling: %lld faces (need at least one)", (long long)nf);
  if (nf > INT32_MAX) return fail(DSDF_E_INVALID, "surface sampling: %lld faces (at most %d)", (long long)nf, INT32_MAX);
  P->tiles = (nf + SURF_TILE - 1) / SURF_TILE;
  P->tile_off = (size_t)rup(nf * 8, 256);
  P->area_off = P->tile_off + (size_t)rup(P->tiles * 8, 256);
  P->bytes = P->area_off + (size_t)rup(nf * 4, 256);
  return 0;
}

SurfBuf surf_buf(void* surf, const SurfPlan& P) {
  SurfBuf b;
  b.cdf = (double*)surf;
  b.tile = (double*)((char*)surf + P.tile_off);
  b.area = (float*)((char*)surf + P.area_off);
  return b;
}
}  // namespace

int dsdf_nn_plan(int64_t n_queries, int64_t n_refs, size_t* ws_bytes, int32_t* n_splits) {
  NnPlan P;
  TRY(nn_plan(n_queries, n_refs, &P, &t_last_plan));
  if (!ws_bytes && !n_splits) return fail(DSDF_E_INVALID, "nearest neighbour plan: every output is NULL");
  if (ws_bytes) *ws_bytes = P.ws;
  if (n_splits) *n_splits = P.n_splits;
  return 0;
}

int dsdf_nn_query(const float* queries, int64_t n_queries, const float* refs, int64_t n_refs, float* sqr_dist, int32_t* index,
                  void* ws, size_t ws_bytes, void* stream) {
  NnPlan P;
  TRY(nn_plan(n_queries, n_refs, &P, &t_last_plan));
  if (!sqr_dist && !index) return fail(DSDF_E_INVALID, "nearest neighbour: every output is NULL");
  if (n_queries == 0) return 0;
  if (!queries || !refs) return fail(DSDF_E_INVALID, "nearest neighbour: NULL queries or reference points");
  if (P.ws && !ws) return fail(DSDF_E_INVALID, "nearest neighbour: NULL workspace");
  if (ws_bytes < P.ws) return fail(DSDF_E_WORKSPACE, "nearest neighbour: workspace %zu < %zu bytes", ws_bytes, P.ws);
  if (P.ws && ((uintptr_t)ws & 3) != 0) return fail(DSDF_E_INVALID, "nearest neighbour: workspace not 4-byte aligned");
  const int nq = (int)n_queries, nr = (int)n_refs;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)P.tiles, (unsigned)P.n_splits);
  if (P.n_splits == 1) {
    hipLaunchKernelGGL((nn_query_kernel<NN_QPL, NN_UNROLL>), grid, dim3(NN_BLOCK), 0, st, refs, nr, P.chunk, queries, nq, sqr_dist, index);
    LAUNCH_OK("nn_query_kernel");
    return 0;
  }
  float* pd2 = (float*)ws;
  int32_t* pidx = (int32_t*)((char*)ws + (size_t)P.n_splits * (size_t)n_queries * 4);
  hipLaunchKernelGGL((nn_query_kernel<NN_QPL, NN_UNROLL>), grid, dim3(NN_BLOCK), 0, st, refs, nr, P.chunk, queries, nq, pd2, pidx);
  LAUNCH_OK("nn_query_kernel");
  hipLaunchKernelGGL(nn_combine_kernel, dim3((unsigned)((n_queries + NN_BLOCK - 1) / NN_BLOCK)), dim3(NN_BLOCK), 0, st,
                     (const float*)pd2, (const int32_t*)pidx, nq, P.n_splits, sqr_dist, index);
  LAUNCH_OK("nn_combine_kernel");
  return 0;
}

int dsdf_mean_f64(const float* x, int64_t n, double* mean, void* ws, size_t ws_bytes, void* stream) {
  static_assert(DSDF_MEAN_WS_BYTES == MEAN_MAX_BLOCKS * 8, "the header's workspace size is the partial-sum table");
  if (n <= 0) return fail(DSDF_E_INVALID, "mean: %lld values (need at least one)", (long long)n);
  if (!x || !mean || !ws) return fail(DSDF_E_INVALID, "mean: NULL values, result or workspace");
  if (ws_bytes < DSDF_MEAN_WS_BYTES) return fail(DSDF_E_WORKSPACE, "mean: workspace %zu < %d bytes", ws_bytes, DSDF_MEAN_WS_BYTES);
  if (((uintptr_t)ws & 7) != 0 || ((uintptr_t)mean & 7) != 0) return fail(DSDF_E_INVALID, "mean: workspace or result not 8-byte aligned");
  const int64_t blocks = std::min<int64_t>((n + MEAN_MIN_SLICE - 1) / MEAN_MIN_SLICE, MEAN_MAX_BLOCKS);
  const int64_t slice = (n + blocks - 1) / blocks;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mean_partial_kernel, dim3((unsigned)blocks), dim3(MEAN_BLOCK), 0, st, x, n, slice, (double*)ws);
  LAUNCH_OK("mean_partial_kernel");
  hipLaunchKernelGGL(mean_final_kernel, dim3(1), dim3(MEAN_BLOCK), 0, st, (const double*)ws, (int)blocks, n, mean);
  LAUNCH_OK("mean_final_kernel");
  return 0;
}

int dsdf_surf_plan(int64_t n_faces, size_t* surf_bytes, size_t* area_offset, int32_t* n_tiles) {
  SurfPlan P;
  TRY(surf_plan(n_faces, &P));
  if (!surf_bytes && !area_offset && !n_tiles) return fail(DSDF_E_INVALID, "surface plan: every output is NULL");
  if (surf_bytes) *surf_bytes = P.bytes;
  if (area_offset) *area_offset = P.area_off;
  if (n_tiles) *n_tiles = (int32_t)P.tiles;
  return 0;
}

namespace {
int surf_args(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const void* surf, size_t surf_bytes,
              SurfPlan* P) {
  TRY(surf_plan(n_faces, P));
  if (n_verts <= 0 || n_verts > INT32_MAX)
    return fail(DSDF_E_INVALID, "surface sampling: %lld vertices (need 1 .. %d)", (long long)n_verts, INT32_MAX);
  if (!verts || !faces || !surf) return fail(DSDF_E_INVALID, "surface sampling: NULL verts, faces or surf buffer");
  if (surf_bytes < P->bytes) return fail(DSDF_E_WORKSPACE, "surface sampling: surf buffer %zu < %zu bytes", surf_bytes, P->bytes);
  if (((uintptr_t)surf & 7) != 0) return fail(DSDF_E_INVALID, "surface sampling: surf buffer not 8-byte aligned");
  return 0;
}
}  // namespace

int dsdf_surf_prepare(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* surf, size_t surf_bytes,
                      double* total_area, void* stream) {
  SurfPlan P;
  TRY(surf_args(verts, n_verts, faces, n_faces, surf, surf_bytes, &P));
  const SurfBuf b = surf_buf(surf, P);
  const int nf = (int)n_faces;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(surf_area_kernel, dim3((unsigned)((n_faces + SURF_BLOCK - 1) / SURF_BLOCK)), dim3(SURF_BLOCK), 0, st, verts,
                     (int)n_verts, faces, nf, b.area);
  LAUNCH_OK("surf_area_kernel");
  hipLaunchKernelGGL(surf_scan_tile_kernel<false>, dim3((unsigned)P.tiles), dim3(SURF_BLOCK), 0, st, b, nf);
  LAUNCH_OK("surf_scan_tile_kernel<false>");
  hipLaunchKernelGGL(surf_scan_tiles_kernel, dim3(1), dim3(SURF_BLOCK), 0, st, b.tile, (int)P.tiles);
  LAUNCH_OK("surf_scan_tiles_kernel");
  hipLaunchKernelGGL(surf_scan_tile_kernel<true>, dim3((unsigned)P.tiles), dim3(SURF_BLOCK), 0, st, b, nf);
  LAUNCH_OK("surf_scan_tile_kernel<true>");
  double total = 0.0;
  HIP_OK(hipMemcpyAsync(&total, b.cdf + (n_faces - 1), sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (total_area) *total_area = total;
  if (!(total > 0.0) || !std::isfinite(total))
    return fail(DSDF_E_INVALID, "surface sampling: the mesh's total area is %g (need a finite positive area)", total);
  return 0;
}

int dsdf_surf_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const void* surf, size_t surf_bytes,
                     int64_t n, uint64_t offset, uint64_t seed, float std_dev, float* points, int32_t* face, float* bary,
                     void* stream) {
  SurfPlan P;
  TRY(surf_args(verts, n_verts, faces, n_faces, surf, surf_bytes, &P));
  if (n < 0 || n > INT32_MAX) return fail(DSDF_E_INVALID, "surface sampling: %lld samples (0 .. %d per call)", (long long)n, INT32_MAX);
  if (offset > UINT64_MAX - (uint64_t)n) return fail(DSDF_E_INVALID, "surface sampling: offset + n exceeds 2^64 - 1");
  if (!(std_dev >= 0.f) || !std::isfinite(std_dev)) return fail(DSDF_E_INVALID, "surface sampling: std must be finite and >= 0");
  if (n == 0) return 0;
  if (!points) return fail(DSDF_E_INVALID, "surface sampling: NULL points");
  SurfOut o;
  o.points = points; o.face = face; o.bary = bary;
  hipLaunchKernelGGL(surf_sample_kernel, dim3((unsigned)((n + SURF_BLOCK - 1) / SURF_BLOCK)), dim3(SURF_BLOCK), 0,
                     (hipStream_t)stream, verts, (int)n_verts, faces, (int)n_faces, (const double*)surf, n, offset, seed, std_dev, o);
  LAUNCH_OK("surf_sample_kernel");
  return 0;
}

// ---- microstructure grids (msgrid.hpp) -------------------------------------------------------------------
namespace {
int ms_grid(const DsdfMsGrid* in, MsGrid* g, int64_t* npts) {
  if (!in) return fail(DSDF_E_INVALID, "microstructure: NULL grid");
  *npts = 1;
  for (int a = 0; a < 3; ++a) {
    const int n = in->dims[a], t = in->tiling[a];
    if (n < 4 || n > MC_MAX_DIM) return fail(DSDF_E_INVALID, "microstructure: padded grid size %d outside 4 .. %d", n, MC_MAX_DIM);
    if (t < 1) return fail(DSDF_E_INVALID, "microstructure: tiling %d < 1", t);
    const double vs = 2.0 / (double)(n - 1 - 2), p = 2.0 / (double)t;
    g->n[a] = n;
    g->vs[a] = (float)vs;
    g->org[a] = (float)(-1.0 - vs);
    g->sub[a] = (float)(t % 2);
    g->mod[a] = (float)(p * 2.0);
    g->p[a] = (float)p;
    g->scale[a] = (float)(2.0 / p);
    *npts *= n;
  }
  return 0;
}

int ms_spline(const DsdfMsSpline* in, MsSpline* s) {
  if (!in) return fail(DSDF_E_INVALID, "microstructure: NULL spline");
  if (in->L < 1) return fail(DSDF_E_INVALID, "microstructure: %d latent columns", in->L);
  int64_t ncp = 1;
  int off = 0;
  for (int a = 0; a < 3; ++a) {
    const int p = in->degree[a], n = in->n_cp[a];
    if (p < 1 || p > MS_MAX_DEG) return fail(DSDF_E_INVALID, "microstructure: degree %d of axis %d outside 1 .. %d", p, a, MS_MAX_DEG);
    if (n <= p || n > (1 << 20)) return fail(DSDF_E_INVALID, "microstructure: %d control points on axis %d (degree %d)", n, a, p);
    if (in->n_knots[a] != n + p + 1)
      return fail(DSDF_E_INVALID, "microstructure: knot vector %d has %d entries, needs n + p + 1 = %d", a, in->n_knots[a], n + p + 1);
    const float* U = in->knots_host[a];
    if (!U) return fail(DSDF_E_INVALID, "microstructure: NULL knot vector %d", a);
    for (int i = 0; i < n + p + 1; ++i) {
      if (!std::isfinite(U[i])) return fail(DSDF_E_INVALID, "microstructure: knot %d of axis %d is not finite", i, a);
      if (i > 0 && U[i] < U[i - 1]) return fail(DSDF_E_INVALID, "microstructure: knot vector %d is decreasing at entry %d", a, i);
    }
    if (!(U[p] < U[n])) return fail(DSDF_E_INVALID, "microstructure: knot vector %d has an empty range", a);
    s->deg[a] = p; s->ncp[a] = n; s->koff[a] = off;
    off += n + p + 1;
    ncp *= n;
  }
  if (in->ncp != ncp) return fail(DSDF_E_INVALID, "microstructure: %lld control points, the axes give %lld", (long long)in->ncp, (long long)ncp);
  if (ncp * (int64_t)in->L > INT32_MAX) return fail(DSDF_E_INVALID, "microstructure: control net of %lld floats (at most %d)", (long long)(ncp * in->L), INT32_MAX);
  if (!in->knots_dev || !in->cp) return fail(DSDF_E_INVALID, "microstructure: NULL device knots or control points");
  s->knots = in->knots_dev; s->cp = in->cp; s->L = in->L;
  return 0;
}
}  // namespace

int dsdf_ms_rows(const DsdfMsSpline* spline, const DsdfMsGrid* grid, int64_t start, int64_t end, const float* points,
                 int32_t inside_test, int32_t with_xyz, float* rows, void* stream) {
  MsGrid g; MsSpline s;
  int64_t npts;
  TRY(ms_grid(grid, &g, &npts));
  TRY(ms_spline(spline, &s));
  if (!rows) return fail(DSDF_E_INVALID, "microstructure rows: NULL rows");
  if (end <= start) return fail(DSDF_E_INVALID, "microstructure rows: empty range [%lld, %lld)", (long long)start, (long long)end);
  if (!points && (start < 0 || end > npts))
    return fail(DSDF_E_INVALID, "microstructure rows: range [%lld, %lld) outside the grid's %lld points", (long long)start, (long long)end, (long long)npts);
  const int64_t n = end - start;
  if (n > INT32_MAX) return fail(DSDF_E_INVALID, "microstructure rows: %lld points in one call (at most %d)", (long long)n, INT32_MAX);
  const int64_t blocks = (n + MS_TILE - 1) / MS_TILE;
  const int64_t first = points ? 0 : start;
  const int test = points ? (int)(inside_test != 0) : 1, xyz = (int)(with_xyz != 0);
  if (s.deg[0] == 1 && s.deg[1] == 1 && s.deg[2] == 1)
    hipLaunchKernelGGL((ms_rows_kernel<true>), dim3((unsigned)blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, g, s, first, n, points,
                       test, xyz, rows);
  else
    hipLaunchKernelGGL((ms_rows_kernel<false>), dim3((unsigned)blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, g, s, first, n, points,
                       test, xyz, rows);
  LAUNCH_OK("ms_rows_kernel");
  return 0;
}

int dsdf_ms_rows_at(const DsdfMsSpline* spline, const DsdfMsGrid* grid, const int64_t* indices, int64_t n, float* rows,
                    float* weights, int32_t* base, void* stream) {
  MsGrid g; MsSpline s;
  int64_t npts;
  TRY(ms_grid(grid, &g, &npts));
  TRY(ms_spline(spline, &s));
  if (n < 0 || n > INT32_MAX) return fail(DSDF_E_INVALID, "microstructure rows at indices: %lld points in one call (0 .. %d)", (long long)n, INT32_MAX);
  if (!indices || !rows) return fail(DSDF_E_INVALID, "microstructure rows at indices: NULL indices or rows");
  if (n == 0) return 0;
  const int64_t blocks = (n + MS_TILE - 1) / MS_TILE;
  if (s.deg[0] == 1 && s.deg[1] == 1 && s.deg[2] == 1)
    hipLaunchKernelGGL((ms_rows_kernel<true, true>), dim3((unsigned)blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, g, s, (int64_t)0, n,
                       (const float*)nullptr, 1, 1, rows, indices, npts, weights, base);
  else
    hipLaunchKernelGGL((ms_rows_kernel<false, true>), dim3((unsigned)blocks), dim3(MS_BLOCK), 0, (hipStream_t)stream, g, s, (int64_t)0, n,
                       (const float*)nullptr, 1, 1, rows, indices, npts, weights, base);
  LAUNCH_OK("ms_rows_kernel(at)");
  return 0;
}

// ---- microstructure mesh derivatives (msdiff.hpp) ----------------------------------------------------------
namespace {
struct MsdPlan { int64_t per; int32_t n_parts, n_tiles; size_t part, ws; };

// What the surface's and the volume's adjoint call things: the messages' prefix and their word for the list, the workspace region
// of the partial sums, the first-stage kernel.
struct MsdNames { const char *what, *verts, *region, *part_kernel; };
constexpr MsdNames MSD_NAMES = {"mesh derivative", "vertices", "msd_vjp_part", "msd_vjp_part_kernel"};
constexpr MsdNames VD_NAMES = {"volume derivative", "moving vertices", "vd_vjp_part", "vd_vjp_part_kernel"};

// The adjoint's workspace for a list of n vertices.
int msd_plan(const MsdNames& N, int64_t n, int64_t ncp, int32_t L, MsdPlan* P, WsTable* rec = nullptr) {
  const char* what = N.what;
  if (n < 0 || n > INT32_MAX) return fail(DSDF_E_INVALID, "%s: %lld %s (0 .. %d)", what, (long long)n, N.verts, INT32_MAX);
  if (L < 1) return fail(DSDF_E_INVALID, "%s: %d latent columns", what, L);
  if (ncp < 1 || ncp * (int64_t)L > INT32_MAX)
    return fail(DSDF_E_INVALID, "%s: control net of %lld x %d floats (1 .. %d)", what, (long long)ncp, L, INT32_MAX);
  P->per = ncp * L;
  P->n_parts = (int32_t)((n + MSD_VJP_VERTS - 1) / MSD_VJP_VERTS);
  P->n_tiles = (int32_t)((P->per + MSD_VJP_TILE - 1) / MSD_VJP_TILE);
  if (P->n_tiles > 65535) return fail(DSDF_E_INVALID, "%s: control net of %lld floats (the adjoint takes at most %lld)", what, (long long)P->per, 65535ll * MSD_VJP_TILE);
  P->part = (size_t)P->n_parts * (size_t)P->per * 4;
  WsCarver c(rec);
  c.take(N.region, -1, P->part);
  P->ws = c.finish(c.o);
  return 0;
}

int msd_plan_out(const MsdNames& N, int64_t n, int64_t ncp, int32_t L, size_t* bytes, int32_t* n_parts) {
  MsdPlan P;
  TRY(msd_plan(N, n, ncp, L, &P, &t_last_plan));
  if (!bytes && !n_parts) return fail(DSDF_E_INVALID, "%s: every output is NULL", N.what);
  if (bytes) *bytes = P.ws;
  if (n_parts) *n_parts = P.n_parts;
  return 0;
}

// The grid of either mesh type: vertex count, sizes and scale -> npts, stride[], scale[].
int msd_grid(int64_t n_verts, const int32_t dims[3], const float scale[3], int64_t* npts, int64_t stride[3], float scale_out[3]) {
  if (n_verts < 0 || n_verts > INT32_MAX)
    return fail(DSDF_E_INVALID, "mesh derivative: %lld vertices (0 .. %d)", (long long)n_verts, INT32_MAX);
  *npts = 1;
  for (int a = 0; a < 3; ++a) {
    const int n = dims[a];
    if (n < 2 || n > MC_MAX_DIM) return fail(DSDF_E_INVALID, "mesh derivative: grid size %d outside 2 .. %d", n, MC_MAX_DIM);
    if (!std::isfinite(scale[a])) return fail(DSDF_E_INVALID, "mesh derivative: scale %d is not finite", a);
    *npts *= n;
    scale_out[a] = scale[a];
  }
  stride[0] = (int64_t)dims[1] * dims[2]; stride[1] = dims[2]; stride[2] = 1;
  return 0;
}

// The band of either mesh type; mesh_ptrs: every per-vertex and per-grid-point array of a mesh that has vertices is there.
int msd_band(const DsdfMsdBand* band, bool has_verts, bool mesh_ptrs, MsdBand* B) {
  if (band->L < 1) return fail(DSDF_E_INVALID, "mesh derivative: %d latent columns", band->L);
  if (band->n_band < 0 || band->n_band > INT32_MAX) return fail(DSDF_E_INVALID, "mesh derivative: %lld band rows", (long long)band->n_band);
  if (band->ld_g < band->L) return fail(DSDF_E_INVALID, "mesh derivative: ld_g %lld < L %d", (long long)band->ld_g, band->L);
  int64_t ncp = 1;
  for (int a = 0; a < 3; ++a) {
    const int p = band->degree[a], n = band->n_cp[a];
    if (p < 1 || p > MS_MAX_DEG) return fail(DSDF_E_INVALID, "mesh derivative: degree %d of axis %d outside 1 .. %d", p, a, MS_MAX_DEG);
    if (n <= p || n > (1 << 20)) return fail(DSDF_E_INVALID, "mesh derivative: %d control points on axis %d (degree %d)", n, a, p);
    B->deg[a] = p; B->ncp[a] = n;
    ncp *= n;
  }
  if (ncp * (int64_t)band->L > INT32_MAX) return fail(DSDF_E_INVALID, "mesh derivative: control net of %lld floats (at most %d)", (long long)(ncp * band->L), INT32_MAX);
  if (has_verts) {
    if (!mesh_ptrs) return fail(DSDF_E_INVALID, "mesh derivative: NULL grid, edge_point, edge_axis or band_of");
    if (band->n_band > 0 && (!band->G || !band->weights || !band->base || !band->mask))
      return fail(DSDF_E_INVALID, "mesh derivative: NULL G, weights, base or mask");
  }
  B->G = band->G; B->w = band->weights; B->base = band->base; B->m = band->mask;
  B->nb = band->n_band; B->ldg = band->ld_g; B->L = band->L; B->ncp_total = (int)ncp;
  return 0;
}

int msd_setup(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, MsdMesh* M, MsdBand* B) {
  if (!mesh || !band) return fail(DSDF_E_INVALID, "mesh derivative: NULL mesh or band");
  TRY(msd_grid(mesh->n_verts, mesh->dims, mesh->scale, &M->npts, M->stride, M->scale));
  TRY(msd_band(band, mesh->n_verts > 0, mesh->grid && mesh->edge_point && mesh->edge_axis && mesh->band_of, B));
  M->grid = mesh->grid; M->edge_point = mesh->edge_point; M->edge_axis = mesh->edge_axis; M->band_of = mesh->band_of;
  M->V = mesh->n_verts; M->level = mesh->level;
  for (int o = 0; o < 2; ++o) msd_magic(M->stride[o], &M->magic[o], &M->shift[o]);
  return 0;
}

// The adjoint of a mesh with a list of n vertices: plan, argument checks, `part` over (parts, tiles) into ws, then the parts summed in
// part order.
extern "C++" template <class Mesh>
int msd_vjp_run(const MsdNames& N, void (*part)(Mesh, MsdBand, const float*, float*), const Mesh& M, int64_t n, const MsdBand& B,
                const float* grad_verts, float* grad_cp, void* ws, size_t ws_bytes, void* stream) {
  MsdPlan P;
  TRY(msd_plan(N, n, B.ncp_total, B.L, &P, &t_last_plan));
  if (!grad_cp) return fail(DSDF_E_INVALID, "%s: NULL grad_cp", N.what);
  if (n > 0 && (!grad_verts || !ws)) return fail(DSDF_E_INVALID, "%s: NULL grad_verts or workspace", N.what);
  if (n > 0 && ws_bytes < P.ws) return fail(DSDF_E_WORKSPACE, "%s: workspace %zu < %zu bytes", N.what, ws_bytes, P.ws);
  hipStream_t st = (hipStream_t)stream;
  if (P.n_parts > 0) {
    hipLaunchKernelGGL(part, dim3((unsigned)P.n_parts, (unsigned)P.n_tiles), dim3(MSD_BLOCK), 0, st, M, B, grad_verts, (float*)ws);
    LAUNCH_OK(N.part_kernel);
  }
  hipLaunchKernelGGL(msd_vjp_sum_kernel, dim3((unsigned)((P.per + MSD_BLOCK - 1) / MSD_BLOCK)), dim3(MSD_BLOCK), 0, st, (const float*)ws,
                     P.n_parts, P.per, grad_cp);
  LAUNCH_OK("msd_vjp_sum_kernel");
  return 0;
}
}  // namespace

int dsdf_msd_vjp_workspace_bytes(int64_t n_verts, int64_t n_control_points, int32_t L, size_t* bytes, int32_t* n_parts) {
  return msd_plan_out(MSD_NAMES, n_verts, n_control_points, L, bytes, n_parts);
}

int dsdf_msd_jacobian(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, int32_t full, float* jac, int32_t* axis, void* stream) {
  MsdMesh M; MsdBand B;
  TRY(msd_setup(mesh, band, &M, &B));
  if (M.V == 0) return 0;
  if (!jac) return fail(DSDF_E_INVALID, "mesh derivative: NULL jacobian");
  const bool vec = B.L % 4 == 0 && (reinterpret_cast<uintptr_t>(jac) & 15) == 0;
  const int64_t stores = (int64_t)B.ncp_total * (B.L / (vec ? 4 : 1)) * (full ? 3 : 1);   // per vertex
  const int vpw = stores >= MSD_DENSE_STORES ? 1 : (int)std::min<int64_t>(MSD_DENSE_VERTS, MSD_DENSE_STORES / stores);
  const dim3 grid((unsigned)((M.V + vpw - 1) / vpw));
  if (vec) hipLaunchKernelGGL((msd_dense_kernel<4>), grid, dim3(MSD_BLOCK), 0, (hipStream_t)stream, M, B, jac, axis, (int)(full != 0), vpw);
  else hipLaunchKernelGGL((msd_dense_kernel<1>), grid, dim3(MSD_BLOCK), 0, (hipStream_t)stream, M, B, jac, axis, (int)(full != 0), vpw);
  LAUNCH_OK("msd_dense_kernel");
  return 0;
}

int dsdf_msd_jvp(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, const float* d_cp, float* d_verts, void* stream) {
  MsdMesh M; MsdBand B;
  TRY(msd_setup(mesh, band, &M, &B));
  if (M.V == 0) return 0;
  if (!d_cp || !d_verts) return fail(DSDF_E_INVALID, "mesh derivative: NULL d_cp or d_verts");
  const int per = MSD_BLOCK / 64;
  hipLaunchKernelGGL(msd_jvp_kernel, dim3((unsigned)((M.V + per - 1) / per)), dim3(MSD_BLOCK), 0, (hipStream_t)stream, M, B, d_cp, d_verts);
  LAUNCH_OK("msd_jvp_kernel");
  return 0;
}

int dsdf_msd_vjp(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, const float* grad_verts, float* grad_cp, void* ws, size_t ws_bytes,
                 void* stream) {
  MsdMesh M; MsdBand B;
  TRY(msd_setup(mesh, band, &M, &B));
  return msd_vjp_run(MSD_NAMES, msd_vjp_part_kernel, M, M.V, B, grad_verts, grad_cp, ws, ws_bytes, stream);
}

// ---- volume mesh derivatives (voldiff.hpp) -------------------------------------------------------------------
namespace {
// grid, scale and band through the surface's checks (the same messages), then the volume mesh's own arrays
int vd_setup(const DsdfVdMesh* mesh, const DsdfMsdBand* band, VdMesh* M, MsdBand* B) {
  if (!mesh || !band) return fail(DSDF_E_INVALID, "volume derivative: NULL mesh or band");
  if (mesh->n_moving < 0 || mesh->n_moving > INT32_MAX)
    return fail(DSDF_E_INVALID, "volume derivative: %lld moving vertices (0 .. %d)", (long long)mesh->n_moving, INT32_MAX);
  if (!(mesh->t_clamp >= 0.f && mesh->t_clamp < 0.5f)) return fail(DSDF_E_INVALID, "volume derivative: t_clamp %g outside [0, 0.5)", (double)mesh->t_clamp);
  TRY(msd_grid(mesh->n_verts, mesh->dims, mesh->scale, &M->npts, M->stride, M->scale));
  TRY(msd_band(band, mesh->n_verts > 0, mesh->grid && mesh->vert_point && mesh->vert_class && mesh->band_of, B));
  if (mesh->n_moving > 0 && (!mesh->vert_index || mesh->n_verts == 0))
    return fail(DSDF_E_INVALID, "volume derivative: NULL vert_index, or moving vertices of an empty mesh");
  M->grid = mesh->grid; M->vert_point = mesh->vert_point; M->vert_class = mesh->vert_class; M->vert_index = mesh->vert_index;
  M->band_of = mesh->band_of;
  M->V = mesh->n_verts; M->Vm = mesh->n_moving; M->level = mesh->level; M->t_clamp = mesh->t_clamp;
  for (int a = 0; a < 3; ++a) M->dims[a] = mesh->dims[a];
  return 0;
}
}  // namespace

int dsdf_vd_vjp_workspace_bytes(int64_t n_moving, int64_t n_control_points, int32_t L, size_t* bytes, int32_t* n_parts) {
  return msd_plan_out(VD_NAMES, n_moving, n_control_points, L, bytes, n_parts);
}

int dsdf_vd_jvp(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* d_cp, float* d_verts, void* stream) {
  VdMesh M; MsdBand B;
  TRY(vd_setup(mesh, band, &M, &B));
  if (M.V == 0) return 0;
  if (!d_verts) return fail(DSDF_E_INVALID, "volume derivative: NULL d_verts");
  if (M.Vm > 0 && !d_cp) return fail(DSDF_E_INVALID, "volume derivative: NULL d_cp");
  hipStream_t st = (hipStream_t)stream;
  HIP_OK(hipMemsetAsync(d_verts, 0, (size_t)M.V * 3 * sizeof(float), st));
  if (M.Vm == 0) return 0;
  const int per = MSD_BLOCK / 64;
  hipLaunchKernelGGL(vd_jvp_kernel, dim3((unsigned)((M.Vm + per - 1) / per)), dim3(MSD_BLOCK), 0, st, M, B, d_cp, d_verts);
  LAUNCH_OK("vd_jvp_kernel");
  return 0;
}

int dsdf_vd_vjp(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* grad_verts, float* grad_cp, void* ws, size_t ws_bytes,
                void* stream) {
  VdMesh M; MsdBand B;
  TRY(vd_setup(mesh, band, &M, &B));
  return msd_vjp_run(VD_NAMES, vd_vjp_part_kernel, M, M.Vm, B, grad_verts, grad_cp, ws, ws_bytes, stream);
}

int dsdf_vd_dtheta(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* normals, const float* stretch, float clip, float* out,
                   void* stream) {
  VdMesh M; MsdBand B;
  TRY(vd_setup(mesh, band, &M, &B));
  if (!stretch) return fail(DSDF_E_INVALID, "volume derivative: NULL stretch");
  VdProject P;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(stretch[a])) return fail(DSDF_E_INVALID, "volume derivative: stretch %d is not finite", a);
    P.stretch[a] = stretch[a];
  }
  if (std::isnan(clip)) return fail(DSDF_E_INVALID, "volume derivative: clip is NaN");
  P.clip = clip;
  if (M.Vm == 0) return 0;
  if (!normals || !out) return fail(DSDF_E_INVALID, "volume derivative: NULL normals or out");
  const int64_t R = (int64_t)B.ncp_total * B.L;
  const int vpw = R >= VD_DENSE_COLS ? 1 : (int)std::min<int64_t>(VD_DENSE_VERTS, VD_DENSE_COLS / R);
  hipLaunchKernelGGL(vd_dtheta_kernel, dim3((unsigned)((M.Vm + vpw - 1) / vpw)), dim3(MSD_BLOCK), 0, (hipStream_t)stream, M, B, normals, P,
                     out, vpw);
  LAUNCH_OK("vd_dtheta_kernel");
  return 0;
}

int dsdf_ms_caps(const DsdfMsGrid* grid, int64_t start, int64_t end, const DsdfMsCap* caps, int32_t n_caps, float* sdf, void* stream) {
  MsGrid g;
  int64_t npts;
  TRY(ms_grid(grid, &g, &npts));
  if (!sdf) return fail(DSDF_E_INVALID, "microstructure caps: NULL sdf");
  if (end <= start || start < 0 || end > npts)
    return fail(DSDF_E_INVALID, "microstructure caps: range [%lld, %lld) empty or outside the grid's %lld points", (long long)start, (long long)end, (long long)npts);
  if (n_caps < 0 || n_caps > MS_MAX_CAPS) return fail(DSDF_E_INVALID, "microstructure caps: %d records (0 .. %d)", n_caps, MS_MAX_CAPS);
  if (n_caps > 0 && !caps) return fail(DSDF_E_INVALID, "microstructure caps: NULL records");
  MsCaps c;
  c.n = n_caps;
  for (int r = 0; r < n_caps; ++r) {
    if (caps[r].dim < 0 || caps[r].dim > 2) return fail(DSDF_E_INVALID, "microstructure caps: record %d names axis %d", r, caps[r].dim);
    if (caps[r].cap != -1 && caps[r].cap != 1) return fail(DSDF_E_INVALID, "microstructure caps: record %d has cap %d (must be -1 or 1)", r, caps[r].cap);
    if (caps[r].m != -1.f && caps[r].m != 1.f) return fail(DSDF_E_INVALID, "microstructure caps: record %d has multiplier %g (must be -1 or 1)", r, (double)caps[r].m);
    if (!std::isfinite(caps[r].c)) return fail(DSDF_E_INVALID, "microstructure caps: record %d has a non-finite plane", r);
    c.r[r].dim = caps[r].dim; c.r[r].cap = caps[r].cap; c.r[r].m = caps[r].m; c.r[r].c = caps[r].c;
  }
  const int64_t n = end - start;
  hipLaunchKernelGGL(ms_caps_kernel, dim3((unsigned)((n + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, (hipStream_t)stream, g, c,
                     start, n, sdf);
  LAUNCH_OK("ms_caps_kernel");
  return 0;
}

}  // extern "C"

// ---- surface topology and geometry (meshtopo.hpp) ----------------------------------------------------------
namespace {
struct MtPlan { int64_t stat_blocks, vol_blocks, vol_slice; size_t stat_off, gf_off, flag_off, vol_off, ws; };
constexpr int64_t MT_MAX_FACES = INT32_MAX / 3;   // a half-edge index 3 f + k is an int32

int mt_plan(int64_t nf, MtPlan* P, WsTable* rec = nullptr) {
  if (nf < 0 || nf > MT_MAX_FACES) return fail(DSDF_E_INVALID, "surface mesh: %lld faces (0 .. %lld)", (long long)nf, (long long)MT_MAX_FACES);
  P->stat_blocks = (3 * nf + MT_BLOCK - 1) / MT_BLOCK;
  P->vol_blocks = std::max<int64_t>(1, std::min<int64_t>((nf + MT_VOL_MIN_SLICE - 1) / MT_VOL_MIN_SLICE, MT_VOL_MAX_BLOCKS));
  P->vol_slice = (nf + P->vol_blocks - 1) / P->vol_blocks;
  WsCarver c(rec);
  P->stat_off = c.take("mt_stat_part", -1, (size_t)std::max<int64_t>(P->stat_blocks, 1) * MT_STATS * 8);
  P->gf_off = c.take("mt_cc_gf", -1, (size_t)std::max<int64_t>(nf, 1) * 4);
  P->flag_off = c.take("mt_cc_flags", -1, (size_t)MT_CC_GROUP * 4);
  P->vol_off = c.take("mt_vol_part", -1, (size_t)MT_VOL_MAX_BLOCKS * 8);
  P->ws = c.finish(c.o);
  return 0;
}

int mt_nverts(int64_t nv) {
  if (nv < 1 || nv > INT32_MAX) return fail(DSDF_E_INVALID, "surface mesh: %lld vertices (1 .. %d)", (long long)nv, INT32_MAX);
  return 0;
}

int mt_ws(const MtPlan& P, const void* ws, size_t ws_bytes) {
  if (!ws) return fail(DSDF_E_INVALID, "surface mesh: NULL workspace");
  if (ws_bytes < P.ws) return fail(DSDF_E_WORKSPACE, "surface mesh: workspace %zu < %zu bytes", ws_bytes, P.ws);
  if (((uintptr_t)ws & 255) != 0) return fail(DSDF_E_INVALID, "surface mesh: workspace not 256-byte aligned");
  return 0;
}

inline dim3 mt_grid(int64_t n) { return dim3((unsigned)((n + MT_BLOCK - 1) / MT_BLOCK)); }

// The host loop of components.hpp over n nodes, after the caller's init kernel: launch_hook(flag) enqueues the caller's hook kernel
// and returns its status.  Waits for the stream: the change flags of every MT_CC_GROUP rounds are read on the host (as
// dsdf_surf_prepare reads its total).  Then the component sizes, if asked for.
template <class Hook>
int cc_run(hipStream_t st, int32_t* label, int32_t* gf, int32_t* flags, int64_t n, Hook launch_hook, int32_t* size, int32_t* n_rounds) {
  const dim3 grid((unsigned)((n + CC_BLOCK - 1) / CC_BLOCK));
  int rounds = 0;
  for (bool done = false; !done;) {                          // no cap: f only decreases, so a round without a change comes
    hipLaunchKernelGGL(cc_flags_kernel, dim3(1), dim3(CC_BLOCK), 0, st, flags);
    LAUNCH_OK("cc_flags_kernel");
    for (int r = 0; r < MT_CC_GROUP; ++r) {
      hipLaunchKernelGGL(cc_grand_kernel, grid, dim3(CC_BLOCK), 0, st, (const int32_t*)label, n, gf);
      LAUNCH_OK("cc_grand_kernel");
      TRY(launch_hook(flags + r));
    }
    int32_t host[MT_CC_GROUP];
    HIP_OK(hipMemcpyAsync(host, flags, sizeof(host), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    for (int r = 0; r < MT_CC_GROUP && !done; ++r) {
      ++rounds;
      done = host[r] == 0;
    }
  }
  if (n_rounds) *n_rounds = rounds;
  if (size) {
    hipLaunchKernelGGL(cc_zero_kernel, grid, dim3(CC_BLOCK), 0, st, size, n);
    LAUNCH_OK("cc_zero_kernel");
    hipLaunchKernelGGL(cc_size_kernel, grid, dim3(CC_BLOCK), 0, st, (const int32_t*)label, n, size);
    LAUNCH_OK("cc_size_kernel");
  }
  return 0;
}
}  // namespace

extern "C" {

int dsdf_mt_plan(int64_t n_verts, int64_t n_faces, size_t* ws_bytes) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P, &t_last_plan));
  if (n_verts < 0 || n_verts > INT32_MAX) return fail(DSDF_E_INVALID, "surface mesh: %lld vertices (0 .. %d)", (long long)n_verts, INT32_MAX);
  if (!ws_bytes) return fail(DSDF_E_INVALID, "surface mesh plan: NULL output");
  *ws_bytes = P.ws;
  return 0;
}

int dsdf_mt_edge_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P));
  TRY(mt_nverts(n_verts));
  if (n_faces == 0) return 0;
  if (!faces || !keys) return fail(DSDF_E_INVALID, "surface mesh: NULL faces or keys");
  hipLaunchKernelGGL(mt_edge_keys_kernel, mt_grid(3 * n_faces), dim3(MT_BLOCK), 0, (hipStream_t)stream, faces, 3 * n_faces, (int)n_verts, keys);
  LAUNCH_OK("mt_edge_keys_kernel");
  return 0;
}

int dsdf_mt_adjacency(const int32_t* faces, int64_t n_faces, const int64_t* sorted_keys, const int64_t* order, int32_t* mate,
                      int64_t* stats, void* ws, size_t ws_bytes, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P, &t_last_plan));
  if (!stats) return fail(DSDF_E_INVALID, "surface mesh: NULL stats");
  TRY(mt_ws(P, ws, ws_bytes));
  if (n_faces == 0) return 0;
  if (!faces || !sorted_keys || !order || !mate) return fail(DSDF_E_INVALID, "surface mesh: NULL faces, keys, order or mate");
  hipStream_t st = (hipStream_t)stream;
  int64_t* part = (int64_t*)((char*)ws + P.stat_off);
  hipLaunchKernelGGL(mt_adjacency_kernel, mt_grid(3 * n_faces), dim3(MT_BLOCK), 0, st, faces, 3 * n_faces, sorted_keys, order, mate, part);
  LAUNCH_OK("mt_adjacency_kernel");
  hipLaunchKernelGGL(mt_stats_sum_kernel, dim3(1), dim3(MT_BLOCK), 0, st, (const int64_t*)part, P.stat_blocks, stats);
  LAUNCH_OK("mt_stats_sum_kernel");
  return 0;
}

int dsdf_mt_components(const int32_t* mate, int64_t n_faces, int32_t* label, int32_t* size, int32_t* n_rounds, void* ws,
                       size_t ws_bytes, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P, &t_last_plan));
  if (n_rounds) *n_rounds = 0;
  if (n_faces == 0) return 0;
  if (!mate || !label) return fail(DSDF_E_INVALID, "surface mesh: NULL mate or label");
  TRY(mt_ws(P, ws, ws_bytes));
  hipStream_t st = (hipStream_t)stream;
  const int nf = (int)n_faces;
  int32_t* gf = (int32_t*)((char*)ws + P.gf_off);
  int32_t* flags = (int32_t*)((char*)ws + P.flag_off);
  const dim3 grid = mt_grid(n_faces);
  hipLaunchKernelGGL(mt_cc_init_kernel, grid, dim3(MT_BLOCK), 0, st, label, nf);
  LAUNCH_OK("mt_cc_init_kernel");
  return cc_run(st, label, gf, flags, n_faces, [&](int32_t* flag) {
    hipLaunchKernelGGL(mt_cc_hook_kernel, grid, dim3(MT_BLOCK), 0, st, mate, nf, label, (const int32_t*)gf, flag);
    LAUNCH_OK("mt_cc_hook_kernel");
    return 0;
  }, size, n_rounds);
}

int dsdf_mt_face_degenerate(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, uint8_t* out, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P));
  TRY(mt_nverts(n_verts));
  if (n_faces == 0) return 0;
  if (!verts || !faces || !out) return fail(DSDF_E_INVALID, "surface mesh: NULL verts, faces or output");
  hipLaunchKernelGGL(mt_degenerate_kernel, mt_grid(n_faces), dim3(MT_BLOCK), 0, (hipStream_t)stream, verts, (int)n_verts, faces, (int)n_faces, out);
  LAUNCH_OK("mt_degenerate_kernel");
  return 0;
}

int dsdf_mt_vertex_geometry(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* corner_order,
                            const int64_t* vstart, float* normals, float* vol_grad, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P));
  TRY(mt_nverts(n_verts));
  if (!normals && !vol_grad) return fail(DSDF_E_INVALID, "surface mesh: every output is NULL");
  if (!verts || !vstart || (n_faces > 0 && (!faces || !corner_order)))
    return fail(DSDF_E_INVALID, "surface mesh: NULL verts, faces, corner_order or vstart");
  hipLaunchKernelGGL(mt_vertex_kernel, mt_grid(n_verts), dim3(MT_BLOCK), 0, (hipStream_t)stream, verts, (int)n_verts, faces, 3 * n_faces,
                     corner_order, vstart, normals, vol_grad);
  LAUNCH_OK("mt_vertex_kernel");
  return 0;
}

int dsdf_mt_volume(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double* volume, void* ws,
                   size_t ws_bytes, void* stream) {
  MtPlan P;
  TRY(mt_plan(n_faces, &P, &t_last_plan));
  TRY(mt_nverts(n_verts));
  if (!volume || ((uintptr_t)volume & 7) != 0) return fail(DSDF_E_INVALID, "surface mesh: NULL or misaligned volume");
  TRY(mt_ws(P, ws, ws_bytes));
  if (n_faces == 0) return 0;
  if (!verts || !faces) return fail(DSDF_E_INVALID, "surface mesh: NULL verts or faces");
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)((char*)ws + P.vol_off);
  hipLaunchKernelGGL(mt_volume_part_kernel, dim3((unsigned)P.vol_blocks), dim3(MT_BLOCK), 0, st, verts, (int)n_verts, faces, n_faces,
                     P.vol_slice, part);
  LAUNCH_OK("mt_volume_part_kernel");
  hipLaunchKernelGGL(mt_volume_final_kernel, dim3(1), dim3(MT_BLOCK), 0, st, (const double*)part, (int)P.vol_blocks, volume);
  LAUNCH_OK("mt_volume_final_kernel");
  return 0;
}

int dsdf_mt_project(const float* jac, const int32_t* axis, const float* normals, int64_t n_verts, int64_t R, const float* stretch,
                    float clip, float* out, void* stream) {
  if (n_verts < 0 || n_verts > INT32_MAX) return fail(DSDF_E_INVALID, "surface mesh: %lld vertices (0 .. %d)", (long long)n_verts, INT32_MAX);
  if (R < 1 || R > INT32_MAX) return fail(DSDF_E_INVALID, "projection: %lld Jacobian columns (1 .. %d)", (long long)R, INT32_MAX);
  if (!stretch) return fail(DSDF_E_INVALID, "projection: NULL stretch");
  MtStretch s;
  for (int a = 0; a < 3; ++a) {
    if (!std::isfinite(stretch[a])) return fail(DSDF_E_INVALID, "projection: stretch %d is not finite", a);
    s.s[a] = stretch[a];
  }
  if (std::isnan(clip)) return fail(DSDF_E_INVALID, "projection: clip is NaN");
  if (n_verts == 0) return 0;
  if (!jac || !axis || !normals || !out) return fail(DSDF_E_INVALID, "projection: NULL jac, axis, normals or out");
  const bool vec = R % 4 == 0 && ((reinterpret_cast<uintptr_t>(jac) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const int64_t Rq = vec ? R / 4 : R, total = n_verts * Rq;
  if ((total + MT_BLOCK - 1) / MT_BLOCK > INT32_MAX) return fail(DSDF_E_INVALID, "projection: %lld x %lld entries in one call", (long long)n_verts, (long long)R);
  if (vec) hipLaunchKernelGGL((mt_project_kernel<4>), mt_grid(total), dim3(MT_BLOCK), 0, (hipStream_t)stream, jac, axis, normals, total, Rq, s, clip, out);
  else hipLaunchKernelGGL((mt_project_kernel<1>), mt_grid(total), dim3(MT_BLOCK), 0, (hipStream_t)stream, jac, axis, normals, total, Rq, s, clip, out);
  LAUNCH_OK("mt_project_kernel");
  return 0;
}

// ---- surface following on blocks of the dense grid (sparsegrid.hpp) ------------------------------------------
// The reference builds the coordinates of all N^3 grid points and decodes every one (deep_sdf/mesh.py:42-70 for create_mesh,
// :262-271 for the microstructure grid); these entries list the points a mesh needs, so that only those are decoded.
namespace {
struct SgPlan {
  SgGrid g;
  int64_t nparts;
  size_t state, pend, have, part, offs, total;
};

int sg_plan(int32_t nx, int32_t ny, int32_t nz, int32_t block, SgPlan* P, WsTable* rec = nullptr) {
  TRY(grid_dims_ok("sparse grid", nx, ny, nz));
  if (block < 2) return fail(DSDF_E_INVALID, "sparse grid: block edge %d < 2 cells", block);
  SgGrid& g = P->g;
  g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  g.b = std::min<int32_t>(block, MC_MAX_DIM);          // an edge past the grid is one block per axis either way
  g.npts = g.nblk = g.ncoarse = 1;
  for (int a = 0; a < 3; ++a) {
    g.nb[a] = (g.n[a] - 1 + g.b - 1) / g.b;
    g.nc[a] = g.nb[a] + 1;
    g.npts *= g.n[a];
    g.nblk *= g.nb[a];
    g.ncoarse *= g.nc[a];
  }
  P->nparts = (g.npts + SG_BLOCK - 1) / SG_BLOCK;      // a per-block pass has no more workgroups: nblk <= npts
  WsCarver c(rec);
  P->state = c.take("sg_state", -1, (size_t)g.nblk);
  P->pend = c.take("sg_pend", -1, (size_t)g.nblk);
  P->have = c.take("sg_have", -1, (size_t)g.npts);
  P->part = c.take("sg_part", -1, (size_t)P->nparts * 4);
  P->offs = c.take("sg_offs", -1, (size_t)(P->nparts + 1) * 8);
  P->total = c.finish(c.o);
  return 0;
}

int sg_setup(int32_t nx, int32_t ny, int32_t nz, int32_t block, void* ws, size_t ws_bytes, SgPlan* P, SgWs* w) {
  TRY(sg_plan(nx, ny, nz, block, P, &t_last_plan));
  if (!ws) return fail(DSDF_E_INVALID, "sparse grid: NULL workspace");
  if (ws_bytes < P->total) return fail(DSDF_E_WORKSPACE, "sparse grid: workspace %zu < %zu bytes", ws_bytes, P->total);
  if (((uintptr_t)ws & 255) != 0) return fail(DSDF_E_INVALID, "sparse grid: workspace not 256-byte aligned");
  char* b = (char*)ws;
  w->state = (uint8_t*)(b + P->state); w->pend = (uint8_t*)(b + P->pend); w->have = (uint8_t*)(b + P->have);
  w->part = (int32_t*)(b + P->part); w->offs = (int64_t*)(b + P->offs);
  w->nparts = P->nparts;
  return 0;
}

inline dim3 sg_launch(int64_t n) { return dim3((unsigned)((n + SG_BLOCK - 1) / SG_BLOCK)); }
}  // namespace

int dsdf_sg_plan(int32_t nx, int32_t ny, int32_t nz, int32_t block, DsdfSgPlan* plan) {
  SgPlan P;
  TRY(sg_plan(nx, ny, nz, block, &P, &t_last_plan));
  if (!plan) return fail(DSDF_E_INVALID, "sparse grid plan: NULL output");
  for (int a = 0; a < 3; ++a) plan->blocks[a] = P.g.nb[a];
  plan->n_blocks = P.g.nblk; plan->n_coarse = P.g.ncoarse; plan->n_points = P.g.npts;
  plan->ws_bytes = P.total;
  plan->state_offset = P.state;
  plan->have_offset = P.have;
  return 0;
}

int dsdf_sg_coarse(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t* indices, void* ws, size_t ws_bytes, void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (!indices) return fail(DSDF_E_INVALID, "sparse grid coarse: NULL indices");
  hipStream_t st = (hipStream_t)stream;
  HIP_OK(hipMemsetAsync(w.have, 0, (size_t)P.g.npts, st));
  hipLaunchKernelGGL(sg_coarse_kernel, sg_launch(P.g.ncoarse), dim3(SG_BLOCK), 0, st, P.g, indices, w.have);
  LAUNCH_OK("sg_coarse_kernel");
  return 0;
}

int dsdf_sg_seed(const float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, float level, float thr, int64_t* n_new, void* ws,
                 size_t ws_bytes, void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (!sdf || !n_new) return fail(DSDF_E_INVALID, "sparse grid seed: NULL sdf or n_new");
  if (!(thr >= 0.f) || !std::isfinite(thr) || std::isnan(level)) return fail(DSDF_E_INVALID, "sparse grid seed: thr %g must be finite and >= 0, level %g a number", (double)thr, (double)level);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = sg_launch(P.g.nblk);
  hipLaunchKernelGGL(sg_seed_kernel, grid, dim3(SG_BLOCK), 0, st, P.g, sdf, level, thr, w.state, w.part);
  LAUNCH_OK("sg_seed_kernel");
  hipLaunchKernelGGL(sg_sum_kernel, dim3(1), dim3(SG_BLOCK), 0, st, (const int32_t*)w.part, (int64_t)grid.x, n_new);
  LAUNCH_OK("sg_sum_kernel");
  return 0;
}

int dsdf_sg_grow(const float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, float level, int64_t* n_new, void* ws,
                 size_t ws_bytes, void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (!sdf || !n_new) return fail(DSDF_E_INVALID, "sparse grid grow: NULL sdf or n_new");
  if (std::isnan(level)) return fail(DSDF_E_INVALID, "sparse grid grow: level is NaN");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid = sg_launch(P.g.nblk);
  hipLaunchKernelGGL(sg_grow_mark_kernel, grid, dim3(SG_BLOCK), 0, st, P.g, sdf, level, (const uint8_t*)w.state, w.pend);
  LAUNCH_OK("sg_grow_mark_kernel");
  hipLaunchKernelGGL(sg_grow_apply_kernel, grid, dim3(SG_BLOCK), 0, st, P.g.nblk, w.state, (const uint8_t*)w.pend, w.part);
  LAUNCH_OK("sg_grow_apply_kernel");
  hipLaunchKernelGGL(sg_sum_kernel, dim3(1), dim3(SG_BLOCK), 0, st, (const int32_t*)w.part, (int64_t)grid.x, n_new);
  LAUNCH_OK("sg_sum_kernel");
  return 0;
}

int dsdf_sg_points_count(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t* n_points, void* ws, size_t ws_bytes, void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (!n_points) return fail(DSDF_E_INVALID, "sparse grid points: NULL n_points");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sg_points_count_kernel, sg_launch(P.g.npts), dim3(SG_BLOCK), 0, st, P.g, (const uint8_t*)w.state, (const uint8_t*)w.have, w.part);
  LAUNCH_OK("sg_points_count_kernel");
  const OffsetScan<1> scan = {{w.part}, {w.offs}, P.nparts, n_points};
  hipLaunchKernelGGL(offset_scan_kernel<1>, dim3(1), dim3(MC_SCAN_THREADS), 0, st, scan);
  LAUNCH_OK("offset_scan_kernel<1>");
  return 0;
}

int dsdf_sg_points_emit(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t n, int64_t* indices, void* ws, size_t ws_bytes,
                        void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (n < 0 || n > P.g.npts) return fail(DSDF_E_INVALID, "sparse grid points: %lld indices (0 .. %lld)", (long long)n, (long long)P.g.npts);
  if (n == 0) return 0;
  if (!indices) return fail(DSDF_E_INVALID, "sparse grid points: NULL indices");
  hipLaunchKernelGGL(sg_points_emit_kernel, sg_launch(P.g.npts), dim3(SG_BLOCK), 0, (hipStream_t)stream, P.g, (const uint8_t*)w.state, w.have,
                     (const int64_t*)w.offs, n, indices);
  LAUNCH_OK("sg_points_emit_kernel");
  return 0;
}

int dsdf_sg_fill(float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, void* ws, size_t ws_bytes, void* stream) {
  SgPlan P; SgWs w;
  TRY(sg_setup(nx, ny, nz, block, ws, ws_bytes, &P, &w));
  if (!sdf) return fail(DSDF_E_INVALID, "sparse grid fill: NULL sdf");
  hipLaunchKernelGGL(sg_fill_kernel, sg_launch(P.g.npts), dim3(SG_BLOCK), 0, (hipStream_t)stream, P.g, (const uint8_t*)w.have, sdf);
  LAUNCH_OK("sg_fill_kernel");
  return 0;
}

int dsdf_sg_coords(int32_t nx, int32_t ny, int32_t nz, const float* voxel_size, const float* origin, const int64_t* indices, int64_t n,
                   float* xyz, void* stream) {
  if (nx < 1 || ny < 1 || nz < 1 || nx > MC_MAX_DIM || ny > MC_MAX_DIM || nz > MC_MAX_DIM)
    return fail(DSDF_E_INVALID, "sparse grid coords: grid %d x %d x %d outside [1, %d] per axis", nx, ny, nz, MC_MAX_DIM);
  if (!voxel_size || !origin) return fail(DSDF_E_INVALID, "sparse grid coords: NULL voxel_size or origin");
  if (n < 0) return fail(DSDF_E_INVALID, "sparse grid coords: %lld indices", (long long)n);
  if (n == 0) return 0;
  if (!indices || !xyz) return fail(DSDF_E_INVALID, "sparse grid coords: NULL indices or xyz");
  SgAxes g;
  g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
  for (int a = 0; a < 3; ++a) { g.vs[a] = voxel_size[a]; g.org[a] = origin[a]; }
  hipLaunchKernelGGL(sg_coords_kernel, sg_launch(n), dim3(SG_BLOCK), 0, (hipStream_t)stream, g, indices, n, xyz);
  LAUNCH_OK("sg_coords_kernel");
  return 0;
}

int dsdf_sg_scatter(const int64_t* indices, int64_t n, const float* values, float* sdf, int64_t n_points, void* stream) {
  if (n < 0 || n_points < 1) return fail(DSDF_E_INVALID, "sparse grid scatter: %lld values into %lld points", (long long)n, (long long)n_points);
  if (n == 0) return 0;
  if (!indices || !values || !sdf) return fail(DSDF_E_INVALID, "sparse grid scatter: NULL indices, values or sdf");
  hipLaunchKernelGGL(sg_scatter_kernel, sg_launch(n), dim3(SG_BLOCK), 0, (hipStream_t)stream, indices, n, values, sdf, n_points);
  LAUNCH_OK("sg_scatter_kernel");
  return 0;
}

int dsdf_sg_caps_at(const DsdfMsGrid* grid, const int64_t* indices, int64_t n, const DsdfMsCap* caps, int32_t n_caps, float* sdf,
                    void* stream) {
  MsGrid g;
  int64_t npts;
  TRY(ms_grid(grid, &g, &npts));
  if (n < 0) return fail(DSDF_E_INVALID, "sparse grid caps: %lld indices", (long long)n);
  if (n_caps < 0 || n_caps > SG_MAX_CAPS) return fail(DSDF_E_INVALID, "sparse grid caps: %d records (0 .. %d)", n_caps, SG_MAX_CAPS);
  if (n_caps > 0 && !caps) return fail(DSDF_E_INVALID, "sparse grid caps: NULL records");
  SgCaps c;
  c.ncaps = n_caps;
  for (int a = 0; a < 3; ++a) { c.n[a] = g.n[a]; c.vs[a] = g.vs[a]; c.org[a] = g.org[a]; }
  for (int r = 0; r < n_caps; ++r) {
    if (caps[r].dim < 0 || caps[r].dim > 2) return fail(DSDF_E_INVALID, "sparse grid caps: record %d names axis %d", r, caps[r].dim);
    if (caps[r].cap != -1 && caps[r].cap != 1) return fail(DSDF_E_INVALID, "sparse grid caps: record %d has cap %d (must be -1 or 1)", r, caps[r].cap);
    if (caps[r].m != -1.f && caps[r].m != 1.f) return fail(DSDF_E_INVALID, "sparse grid caps: record %d has multiplier %g (must be -1 or 1)", r, (double)caps[r].m);
    if (!std::isfinite(caps[r].c)) return fail(DSDF_E_INVALID, "sparse grid caps: record %d has a non-finite plane", r);
    c.r[r].dim = caps[r].dim; c.r[r].cap = caps[r].cap; c.r[r].m = caps[r].m; c.r[r].c = caps[r].c;
  }
  if (n == 0) return 0;
  if (!indices || !sdf) return fail(DSDF_E_INVALID, "sparse grid caps: NULL indices or sdf");
  hipLaunchKernelGGL(sg_caps_kernel, sg_launch(n), dim3(SG_BLOCK), 0, (hipStream_t)stream, c, indices, n, sdf);
  LAUNCH_OK("sg_caps_kernel");
  return 0;
}

// ---- tetrahedral volume mesh (tetmesh.hpp) ---------------------------------------------------------------------
namespace {
struct TetPlan {
  int64_t npts, nblocks;
  size_t rec, ne, nb, vbase, bcount[3], boff[3], gf, flags, total;
};

int tet_plan(int32_t nx, int32_t ny, int32_t nz, TetPlan* P, WsTable* rec = nullptr) {
  TRY(grid_dims_ok("tet mesh", nx, ny, nz));
  P->npts = (int64_t)nx * ny * nz;
  P->nblocks = (P->npts + TET_BLOCK - 1) / TET_BLOCK;
  WsCarver c(rec);
  P->rec = c.take("tet_rec", -1, (size_t)P->npts);
  P->ne = c.take("tet_ne", -1, (size_t)P->npts);
  P->nb = c.take("tet_nb", -1, (size_t)P->npts);
  P->vbase = c.take("tet_vbase", -1, (size_t)P->npts * 4);
  static const char* const cnt_name[3] = {"tet_bv", "tet_bt", "tet_bb"};
  static const char* const off_name[3] = {"tet_ov", "tet_ot", "tet_ob"};
  for (int s = 0; s < 3; ++s) P->bcount[s] = c.take(cnt_name[s], -1, (size_t)P->nblocks * 4);
  for (int s = 0; s < 3; ++s) P->boff[s] = c.take(off_name[s], -1, (size_t)(P->nblocks + 1) * 8);
  P->gf = c.take("tet_cc_gf", -1, (size_t)P->npts * 4);
  P->flags = c.take("tet_cc_flags", -1, (size_t)MT_CC_GROUP * 4);
  P->total = c.finish(c.o);
  return 0;
}

int tet_setup(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, void* ws, size_t ws_bytes, McGrid* g, TetWs* w,
              TetPlan* P) {
  TRY(tet_plan(nx, ny, nz, P, &t_last_plan));
  if (!sdf || !ws) return fail(DSDF_E_INVALID, "tet mesh: NULL sdf or workspace");
  if (ws_bytes < P->total) return fail(DSDF_E_WORKSPACE, "tet mesh: workspace %zu < %zu bytes", ws_bytes, P->total);
  g->sdf = sdf; g->nx = nx; g->ny = ny; g->nz = nz; g->level = level; g->npts = P->npts;
  char* b = (char*)ws;
  w->rec = (uint8_t*)(b + P->rec); w->ne = (uint8_t*)(b + P->ne); w->nb = (uint8_t*)(b + P->nb);
  w->vbase = (int32_t*)(b + P->vbase);
  for (int s = 0; s < 3; ++s) { w->bcount[s] = (int32_t*)(b + P->bcount[s]); w->boff[s] = (int64_t*)(b + P->boff[s]); }
  w->nblocks = P->nblocks;
  return 0;
}
}  // namespace

int dsdf_tet_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes) {
  TetPlan P;
  TRY(tet_plan(nx, ny, nz, &P, &t_last_plan));
  if (!bytes) return fail(DSDF_E_INVALID, "NULL bytes");
  *bytes = P.total;
  return 0;
}

int dsdf_tet_count(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* totals, void* ws, size_t ws_bytes,
                   void* stream) {
  McGrid g; TetWs w; TetPlan P;
  TRY(tet_setup(sdf, nx, ny, nz, level, ws, ws_bytes, &g, &w, &P));
  if (!totals) return fail(DSDF_E_INVALID, "tet mesh: NULL totals");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tet_classify_kernel, dim3((unsigned)P.nblocks), dim3(TET_BLOCK), 0, st, g, w);
  LAUNCH_OK("tet_classify_kernel");
  const OffsetScan<3> scan = {{w.bcount[0], w.bcount[1], w.bcount[2]}, {w.boff[0], w.boff[1], w.boff[2]}, w.nblocks, totals};
  hipLaunchKernelGGL(offset_scan_kernel<3>, dim3(1), dim3(MC_SCAN_THREADS), 0, st, scan);
  LAUNCH_OK("offset_scan_kernel<3>");
  return 0;
}

int dsdf_tet_emit(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing, const float* origin,
                  float t_clamp, int64_t n_verts, int64_t n_tets, int64_t n_bfaces, float* verts, int32_t* tets, int32_t* bfaces,
                  int8_t* bface_kind, int64_t* vert_point, int32_t* vert_class, void* ws, size_t ws_bytes, void* stream) {
  McGrid g; TetWs w; TetPlan P;
  TRY(tet_setup(sdf, nx, ny, nz, level, ws, ws_bytes, &g, &w, &P));
  if (!(t_clamp >= 0.f && t_clamp < 0.5f)) return fail(DSDF_E_INVALID, "tet mesh: t_clamp %g outside [0, 0.5)", (double)t_clamp);
  if (n_verts < 0 || n_tets < 0 || n_bfaces < 0 || n_verts > INT32_MAX || n_tets > INT32_MAX || n_bfaces > INT32_MAX)
    return fail(DSDF_E_INVALID, "tet mesh: %lld vertices / %lld elements / %lld boundary triangles (int32 indices hold at most %d)",
                (long long)n_verts, (long long)n_tets, (long long)n_bfaces, INT32_MAX);
  if (!spacing || !origin) return fail(DSDF_E_INVALID, "tet mesh: NULL spacing or origin");
  if ((n_verts > 0 && !verts) || (n_tets > 0 && !tets) || (n_bfaces > 0 && (!bfaces || !bface_kind)))
    return fail(DSDF_E_INVALID, "tet mesh: NULL verts, tets, bfaces or bface_kind");
  if (((uintptr_t)tets & 15) != 0) return fail(DSDF_E_INVALID, "tet mesh: tets not 16-byte aligned (an element is stored as one int4)");
  if (n_verts == 0 && n_tets == 0 && n_bfaces == 0) return 0;
  TetOut o;
  for (int a = 0; a < 3; ++a) { o.spacing[a] = spacing[a]; o.origin[a] = origin[a]; }
  o.t_clamp = t_clamp;
  o.verts = verts; o.tets = tets; o.bfaces = bfaces; o.bface_kind = bface_kind; o.vert_point = vert_point; o.vert_class = vert_class;
  o.nv = n_verts; o.nt = n_tets; o.nb = n_bfaces;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tet_vertex_kernel, dim3((unsigned)P.nblocks), dim3(TET_BLOCK), 0, st, g, w, o);
  LAUNCH_OK("tet_vertex_kernel");
  if (n_tets > 0 || n_bfaces > 0) {
    hipLaunchKernelGGL(tet_element_kernel, dim3((unsigned)P.nblocks), dim3(TET_BLOCK), 0, st, g, w, o);
    LAUNCH_OK("tet_element_kernel");
  }
  return 0;
}

int dsdf_tet_components(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int32_t* label, int32_t* size,
                        int32_t* n_rounds, void* ws, size_t ws_bytes, void* stream) {
  McGrid g; TetWs w; TetPlan P;
  if (n_rounds) *n_rounds = 0;
  TRY(tet_setup(sdf, nx, ny, nz, level, ws, ws_bytes, &g, &w, &P));
  if (!label) return fail(DSDF_E_INVALID, "tet mesh components: NULL label");
  hipStream_t st = (hipStream_t)stream;
  int32_t* gf = (int32_t*)((char*)ws + P.gf);
  int32_t* flags = (int32_t*)((char*)ws + P.flags);
  const dim3 grid((unsigned)P.nblocks);
  hipLaunchKernelGGL(tet_cc_init_kernel, grid, dim3(TET_BLOCK), 0, st, g, label);
  LAUNCH_OK("tet_cc_init_kernel");
  return cc_run(st, label, gf, flags, P.npts, [&](int32_t* flag) {
    hipLaunchKernelGGL(tet_cc_hook_kernel, grid, dim3(TET_BLOCK), 0, st, g, label, (const int32_t*)gf, flag);
    LAUNCH_OK("tet_cc_hook_kernel");
    return 0;
  }, size, n_rounds);
}

// ---- P1 linear elasticity (fem.hpp) -----------------------------------------------------------------------------------
namespace {
struct FemPlan {
  int64_t nbv, nbe, npart;
  size_t sig, r, z, p, ap, part[2], cnt, scal, total;
};

int fem_plan(int64_t nv, int64_t nt, int64_t nb, FemPlan* P, WsTable* rec = nullptr) {
  if (nv < 1 || nt < 1 || nb < 0 || nv > INT32_MAX || nt > INT32_MAX / 4 || nb > INT32_MAX / 3)
    return fail(DSDF_E_INVALID, "fem: %lld vertices / %lld elements / %lld boundary triangles (need >= 1 vertex and element; corners fit int32)",
                (long long)nv, (long long)nt, (long long)nb);
  P->nbv = (nv + FEM_BLOCK - 1) / FEM_BLOCK;
  P->nbe = (nt + FEM_BLOCK - 1) / FEM_BLOCK;
  P->npart = std::max(P->nbv, P->nbe);
  WsCarver c(rec);
  P->sig = c.take("fem_sigma", -1, (size_t)nt * 6 * 8);
  P->r = c.take("fem_r", -1, (size_t)nv * 3 * 8);
  P->z = c.take("fem_z", -1, (size_t)nv * 3 * 8);
  P->p = c.take("fem_p", -1, (size_t)nv * 3 * 8);
  P->ap = c.take("fem_ap", -1, (size_t)nv * 3 * 8);
  P->part[0] = c.take("fem_part0", -1, (size_t)P->npart * 8);
  P->part[1] = c.take("fem_part1", -1, (size_t)P->npart * 8);
  P->cnt = c.take("fem_cnt", -1, (size_t)P->npart * 4);
  P->scal = c.take("fem_scal", -1, sizeof(FemScal));
  P->total = c.finish(c.o);
  return 0;
}

// The checks every entry that takes an operator shares, the plan it records, and the kernels' view of the operator.
int fem_op(const char* what, const DsdfFemOp* op, void* ws, size_t ws_bytes, FemPlan* P, FemMesh* m) {
  if (!op) return fail(DSDF_E_INVALID, "%s: NULL operator", what);
  TRY(fem_plan(op->n_verts, op->n_tets, 0, P, &t_last_plan));
  if (!op->tets || !op->corner_order || !op->vstart || !op->geom || !op->dinv || !op->mask)
    return fail(DSDF_E_INVALID, "%s: NULL tets, corner_order, vstart, geom, dinv or mask", what);
  if (!aligned16(op->tets)) return fail(DSDF_E_INVALID, "%s: tets not 16-byte aligned (an element is read as one int4)", what);
  if (!std::isfinite(op->lam) || !std::isfinite(op->mu) || !(op->mu > 0.0) || !(op->lam + 2.0 * op->mu > 0.0))
    return fail(DSDF_E_INVALID, "%s: lam %g, mu %g (need finite values, mu > 0, lam + 2 mu > 0)", what, op->lam, op->mu);
  if (!ws) return fail(DSDF_E_INVALID, "%s: NULL workspace", what);
  if (ws_bytes < P->total) return fail(DSDF_E_WORKSPACE, "%s: workspace %zu < %zu bytes", what, ws_bytes, P->total);
  if (((uintptr_t)ws & 255) != 0) return fail(DSDF_E_INVALID, "%s: workspace not 256-byte aligned", what);
  m->tets = op->tets; m->corder = op->corner_order; m->vstart = op->vstart; m->geom = op->geom; m->mask = op->mask;
  m->nt = op->n_tets; m->nv = op->n_verts; m->lam = op->lam; m->mu = op->mu;
  return 0;
}

int fem_boundary_args(const char* what, const double* verts, int64_t nv, const int32_t* bfaces, int64_t nb, const int64_t* border,
                      const int64_t* bvstart, const double* out) {
  if (nv < 1 || nb < 0 || nv > INT32_MAX || nb > INT32_MAX / 3)
    return fail(DSDF_E_INVALID, "%s: %lld vertices / %lld boundary triangles", what, (long long)nv, (long long)nb);
  if (!verts || !bvstart || !out || (nb > 0 && (!bfaces || !border)))
    return fail(DSDF_E_INVALID, "%s: NULL verts, bfaces, bcorner_order, bvstart or output", what);
  return 0;
}

inline dim3 fem_grid(int64_t n) { return dim3((unsigned)((n + FEM_BLOCK - 1) / FEM_BLOCK)); }

// y = A x on the stream: the two passes; part / scal as in fem_gather_kernel
int fem_apply_launch(const FemMesh& m, const FemPlan& P, char* b, const double* x, double* y, double* part, const FemScal* scal,
                     hipStream_t st) {
  double* sig = (double*)(b + P.sig);
  hipLaunchKernelGGL(fem_stress_kernel, fem_grid(m.nt), dim3(FEM_BLOCK), 0, st, m, x, sig, scal);
  LAUNCH_OK("fem_stress_kernel");
  hipLaunchKernelGGL(fem_gather_kernel, fem_grid(m.nv), dim3(FEM_BLOCK), 0, st, m, (const double*)sig, x, y, part, scal);
  LAUNCH_OK("fem_gather_kernel");
  return 0;
}
}  // namespace

int dsdf_fem_plan(int64_t n_verts, int64_t n_tets, int64_t n_bfaces, size_t* ws_bytes) {
  FemPlan P;
  TRY(fem_plan(n_verts, n_tets, n_bfaces, &P, &t_last_plan));
  if (!ws_bytes) return fail(DSDF_E_INVALID, "fem plan: NULL ws_bytes");
  *ws_bytes = P.total;
  return 0;
}

int dsdf_fem_setup(const DsdfFemOp* op, const double* verts, const uint8_t* fixed, double* diag, int64_t* counts, void* ws,
                   size_t ws_bytes, void* stream) {
  FemPlan P; FemMesh m;
  TRY(fem_op("fem setup", op, ws, ws_bytes, &P, &m));
  if (!verts || !diag || !counts) return fail(DSDF_E_INVALID, "fem setup: NULL verts, diag or counts");
  hipStream_t st = (hipStream_t)stream;
  int32_t* cnt = (int32_t*)((char*)ws + P.cnt);
  hipLaunchKernelGGL(fem_geom_kernel, fem_grid(m.nt), dim3(FEM_BLOCK), 0, st, verts, m.nv, m.tets, m.nt, (double*)op->geom, cnt);
  LAUNCH_OK("fem_geom_kernel");
  hipLaunchKernelGGL(fem_count_final_kernel, dim3(1), dim3(FEM_BLOCK), 0, st, (const int32_t*)cnt, P.nbe, counts);
  LAUNCH_OK("fem_count_final_kernel");
  hipLaunchKernelGGL(fem_diag_kernel, fem_grid(m.nv), dim3(FEM_BLOCK), 0, st, m, fixed, diag, (double*)op->dinv, (uint8_t*)op->mask, cnt);
  LAUNCH_OK("fem_diag_kernel");
  hipLaunchKernelGGL(fem_count_final_kernel, dim3(1), dim3(FEM_BLOCK), 0, st, (const int32_t*)cnt, P.nbv, counts + 1);
  LAUNCH_OK("fem_count_final_kernel");
  return 0;
}

int dsdf_fem_apply(const DsdfFemOp* op, const double* x, double* y, void* ws, size_t ws_bytes, void* stream) {
  FemPlan P; FemMesh m;
  TRY(fem_op("fem apply", op, ws, ws_bytes, &P, &m));
  if (!x || !y || x == y) return fail(DSDF_E_INVALID, "fem apply: NULL x or y, or x == y");
  return fem_apply_launch(m, P, (char*)ws, x, y, nullptr, nullptr, (hipStream_t)stream);
}

int dsdf_fem_load(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                  const int64_t* bvstart, const uint8_t* face_sel, const double* traction, const uint8_t* mask, double* f, void* stream) {
  TRY(fem_boundary_args("fem load", verts, n_verts, bfaces, n_bfaces, bcorner_order, bvstart, f));
  if (!traction || !std::isfinite(traction[0]) || !std::isfinite(traction[1]) || !std::isfinite(traction[2]))
    return fail(DSDF_E_INVALID, "fem load: NULL or non-finite traction");
  hipLaunchKernelGGL(fem_boundary_kernel<true>, fem_grid(n_verts), dim3(FEM_BLOCK), 0, (hipStream_t)stream, verts, n_verts, bfaces, n_bfaces,
                     bcorner_order, bvstart, face_sel, traction[0], traction[1], traction[2], mask, (const double*)nullptr, f);
  LAUNCH_OK("fem_boundary_kernel<load>");
  return 0;
}

int dsdf_fem_boundary_gradient(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                               const int64_t* bvstart, const double* weight, double* grad, void* stream) {
  TRY(fem_boundary_args("fem boundary gradient", verts, n_verts, bfaces, n_bfaces, bcorner_order, bvstart, grad));
  hipLaunchKernelGGL(fem_boundary_kernel<false>, fem_grid(n_verts), dim3(FEM_BLOCK), 0, (hipStream_t)stream, verts, n_verts, bfaces, n_bfaces,
                     bcorner_order, bvstart, (const uint8_t*)nullptr, 0.0, 0.0, 0.0, (const uint8_t*)nullptr, weight, grad);
  LAUNCH_OK("fem_boundary_kernel<gradient>");
  return 0;
}

int dsdf_fem_solve(const DsdfFemOp* op, const double* f, double* u, double rel_tol, int32_t max_iter, int32_t check_every,
                   int32_t* iterations, int32_t* converged, double* ratio, void* ws, size_t ws_bytes, void* stream) {
  FemPlan P; FemMesh m;
  if (iterations) *iterations = 0;
  if (converged) *converged = 0;
  if (ratio) *ratio = 0.0;
  TRY(fem_op("fem solve", op, ws, ws_bytes, &P, &m));
  if (!f || !u || f == u) return fail(DSDF_E_INVALID, "fem solve: NULL f or u, or f == u");
  if (!(rel_tol >= 0.0) || !std::isfinite(rel_tol)) return fail(DSDF_E_INVALID, "fem solve: rel_tol %g must be finite and >= 0", rel_tol);
  if (max_iter < 0 || check_every < 1) return fail(DSDF_E_INVALID, "fem solve: max_iter %d < 0 or check_every %d < 1", max_iter, check_every);
  hipStream_t st = (hipStream_t)stream;
  char* b = (char*)ws;
  double *r = (double*)(b + P.r), *z = (double*)(b + P.z), *p = (double*)(b + P.p), *ap = (double*)(b + P.ap);
  double *part0 = (double*)(b + P.part[0]), *part1 = (double*)(b + P.part[1]);
  FemScal* s = (FemScal*)(b + P.scal);
  const dim3 gv = fem_grid(m.nv), one(1), blk(FEM_BLOCK);
  hipLaunchKernelGGL(fem_cg_start_kernel, gv, blk, 0, st, m.nv, m.mask, op->dinv, f, u, r, z, p, part1);
  LAUNCH_OK("fem_cg_start_kernel");
  hipLaunchKernelGGL(fem_cg_init_kernel, one, blk, 0, st, (const double*)part1, P.nbv, s, rel_tol * rel_tol);
  LAUNCH_OK("fem_cg_init_kernel");
  FemScal h;
  for (int32_t i = 0; i < max_iter; ++i) {
    TRY(fem_apply_launch(m, P, b, p, ap, part0, s, st));
    hipLaunchKernelGGL(fem_cg_alpha_kernel, one, blk, 0, st, (const double*)part0, P.nbv, s);
    LAUNCH_OK("fem_cg_alpha_kernel");
    hipLaunchKernelGGL(fem_cg_update_kernel, gv, blk, 0, st, m.nv, op->dinv, (const FemScal*)s, (const double*)p, (const double*)ap, u, r, z, part1);
    LAUNCH_OK("fem_cg_update_kernel");
    hipLaunchKernelGGL(fem_cg_beta_kernel, one, blk, 0, st, (const double*)part1, P.nbv, s);
    LAUNCH_OK("fem_cg_beta_kernel");
    hipLaunchKernelGGL(fem_cg_dir_kernel, fem_grid(m.nv * 3), blk, 0, st, m.nv * 3, (const FemScal*)s, (const double*)z, p);
    LAUNCH_OK("fem_cg_dir_kernel");
    if ((i + 1) % check_every == 0 && i + 1 < max_iter) {
      HIP_OK(hipMemcpyAsync(&h, s, sizeof(h), hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      if (h.done) break;
    }
  }
  HIP_OK(hipMemcpyAsync(&h, s, sizeof(h), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  if (iterations) *iterations = h.it;
  if (converged) *converged = h.converged;
  if (ratio) *ratio = h.rho0 > 0.0 ? h.rho / h.rho0 : 0.0;
  return 0;
}

int dsdf_fem_energy(const DsdfFemOp* op, const double* u, double* we, int32_t nodal, double* wv, double* totals, void* ws,
                    size_t ws_bytes, void* stream) {
  FemPlan P; FemMesh m;
  TRY(fem_op("fem energy", op, ws, ws_bytes, &P, &m));
  if (!u || !we || !totals) return fail(DSDF_E_INVALID, "fem energy: NULL u, we or totals");
  if (nodal < 0 || nodal > FEM_NODAL_LAST || (nodal != 0) != (wv != nullptr))
    return fail(DSDF_E_INVALID, "fem energy: nodal %d (0: none, 1: mean, 2: last) and wv must come together", nodal);
  hipStream_t st = (hipStream_t)stream;
  char* b = (char*)ws;
  double *part0 = (double*)(b + P.part[0]), *part1 = (double*)(b + P.part[1]);
  hipLaunchKernelGGL(fem_energy_elem_kernel, fem_grid(m.nt), dim3(FEM_BLOCK), 0, st, m, u, we, part0, part1);
  LAUNCH_OK("fem_energy_elem_kernel");
  hipLaunchKernelGGL(fem_sum_final_kernel, dim3(1), dim3(FEM_BLOCK), 0, st, (const double*)part0, P.nbe, totals);
  LAUNCH_OK("fem_sum_final_kernel");
  hipLaunchKernelGGL(fem_sum_final_kernel, dim3(1), dim3(FEM_BLOCK), 0, st, (const double*)part1, P.nbe, totals + 1);
  LAUNCH_OK("fem_sum_final_kernel");
  if (nodal) {
    hipLaunchKernelGGL(fem_energy_vertex_kernel, fem_grid(m.nv), dim3(FEM_BLOCK), 0, st, m, (const double*)we, (int)nodal, wv);
    LAUNCH_OK("fem_energy_vertex_kernel");
  }
  return 0;
}

int dsdf_fem_stiffness_gradient(const DsdfFemOp* op, const double* u, double* emt, double* grad, void* ws, size_t ws_bytes, void* stream) {
  FemPlan P; FemMesh m;
  TRY(fem_op("fem stiffness gradient", op, ws, ws_bytes, &P, &m));
  if (!u || !emt || !grad) return fail(DSDF_E_INVALID, "fem stiffness gradient: NULL u, emt or grad");
  if (u == grad || u == emt || emt == grad) return fail(DSDF_E_INVALID, "fem stiffness gradient: u == grad, u == emt or emt == grad");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(fem_emt_kernel, fem_grid(m.nt), dim3(FEM_BLOCK), 0, st, m, u, emt);
  LAUNCH_OK("fem_emt_kernel");
  hipLaunchKernelGGL(fem_emt_gather_kernel, fem_grid(m.nv), dim3(FEM_BLOCK), 0, st, m, (const double*)emt, grad);
  LAUNCH_OK("fem_emt_gather_kernel");
  return 0;
}

int dsdf_fem_load_gradient(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                           const int64_t* bvstart, const uint8_t* face_sel, const double* traction, const uint8_t* mask, const double* u,
                           double* grad, void* stream) {
  TRY(fem_boundary_args("fem load gradient", verts, n_verts, bfaces, n_bfaces, bcorner_order, bvstart, grad));
  if (!u) return fail(DSDF_E_INVALID, "fem load gradient: NULL u");
  if (u == grad) return fail(DSDF_E_INVALID, "fem load gradient: u == grad");
  if (!traction || !std::isfinite(traction[0]) || !std::isfinite(traction[1]) || !std::isfinite(traction[2]))
    return fail(DSDF_E_INVALID, "fem load gradient: NULL or non-finite traction");
  hipLaunchKernelGGL(fem_load_gradient_kernel, fem_grid(n_verts), dim3(FEM_BLOCK), 0, (hipStream_t)stream, verts, n_verts, bfaces, n_bfaces,
                     bcorner_order, bvstart, face_sel, traction[0], traction[1], traction[2], mask, u, grad);
  LAUNCH_OK("fem_load_gradient_kernel");
  return 0;
}

}  // extern "C"

// Last function of the translation unit's device code: warm_own_code (common.hpp) clamps its reads to this address.
namespace dsdf {
__device__ __noinline__ void dsdf_text_end_marker() { asm volatile("s_nop 0"); }
}  // namespace dsdf
