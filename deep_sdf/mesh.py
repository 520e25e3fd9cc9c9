"""Import-name shim: ``import deep_sdf.mesh`` (create_ply_files_from_latent.py:1, reconstruction scripts) resolves to the GPU
meshing of deepsdf_amd/mesh.py (HIP marching cubes, in-house PLY writer, microstructure rows and caps in HIP)."""
from deepsdf_amd.mesh import convert_sdf_samples_to_ply, create_mesh  # noqa: F401
from deepsdf_amd.mesh import (CapBorderDict, CapType, create_mesh_microstructure, location_lookup,  # noqa: F401
                              microstructure_sdf_grid, sdf_struct)
