"""Import-name shim: ``deep_sdf.metrics.chamfer`` resolves to the GPU implementation (deepsdf_amd/metrics.py)."""
from . import chamfer  # noqa: F401
