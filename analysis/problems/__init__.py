"""The reference's ``analysis.problems`` package name: the load cases of the optimisation loop on deepsdf_amd.fem."""
