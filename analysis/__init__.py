"""The reference's ``analysis`` package name: ``analysis.geometry.DeepSDFMesh`` on the GPU (deepsdf_amd.surface)."""
