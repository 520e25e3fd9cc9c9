"""Import-name shim: ``import deep_sdf.mesh`` (create_ply_files_from_latent.py:1, reconstruction scripts) resolves to the GPU
meshing of deepsdf_amd/mesh.py (HIP marching cubes, in-house PLY writer)."""
from deepsdf_amd.mesh import convert_sdf_samples_to_ply, create_mesh  # noqa: F401
