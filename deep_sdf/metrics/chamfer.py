"""``deep_sdf/metrics/chamfer.py`` of the reference: compute_trimesh_chamfer, computed on the GPU without trimesh or scipy."""
from deepsdf_amd.metrics import compute_trimesh_chamfer  # noqa: F401

__all__ = ["compute_trimesh_chamfer"]
