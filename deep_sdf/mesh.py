"""Import-name shim: ``import deep_sdf.mesh`` (create_ply_files_from_latent.py:1, reconstruction scripts) resolves to the GPU
meshing of deepsdf_amd/mesh.py (HIP marching cubes, in-house PLY writer, microstructure rows and caps in HIP, mesh derivatives with
respect to the spline's control points assembled in HIP)."""
from deepsdf_amd.mesh import convert_sdf_samples_to_ply, create_mesh  # noqa: F401
from deepsdf_amd.mesh import (CapBorderDict, CapType, create_mesh_microstructure, create_mesh_microstructure_diff,  # noqa: F401
                              location_lookup, microstructure_mesh_diff, microstructure_sdf_grid, sdf_struct, sparse_grid)
from deepsdf_amd.mesh import add_sparse_args  # noqa: F401
from deepsdf_amd.mesh import TetMesh, microstructure_tetmesh, solid_components, tetrahedralize  # noqa: F401
