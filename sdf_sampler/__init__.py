"""Import-name shim: ``from sdf_sampler import sdf_sampler`` (the reference's data scripts, e.g.
evaluation_scripts/10_gen_double_lattice_training_data.py) resolves to deepsdf_amd/sdf_sampler.py, whose ``SDFfromMesh`` runs
on the GPU.  The reference's splinepy/gustaf tile generators (microstructures, double_lattice_extruded, snappy_3d) are not
part of this package."""
