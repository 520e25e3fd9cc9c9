"""The optimisation loop around analysis/: control points -> surface -> volume mesh -> elasticity -> (compliance, volume) and their
gradients (optimization.opti.struct_optimization)."""
