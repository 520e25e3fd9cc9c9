"""The reference's ``optimization/opti.py`` evaluation step and scipy driver on the GPU stages of this package.

One evaluation (``_compute_solution``): control points -> DeepSDFMesh.generate_surface_mesh -> generate_volume_mesh ->
CantileverBeam.set_mesh / set_up -> volume and its gradient -> solve -> compliance and its gradient.  The mesh stays on the device
between the stages: nothing is written but ``results.json``.  By default the gradients come from the adjoint
(DeepSDFMesh.shape_gradient: no dense array, no outlier clipping); ``general.dense_dtheta`` = true builds the reference's dense
``get_dTheta()`` (with its clipping) and contracts it, as the reference does.

Not here: the MMA method (it needs the mmapy package), plotting and animation."""
import dataclasses
import json
import logging
import os
import pathlib

import numpy as np

from analysis.geometry import DeepSDFMesh
from analysis.problems.CantileverBeam import CantileverBeam
from optimization import config

METHODS = ("BFGS", "COBYLA", "MMA")                  # what config.json may name; MMA is refused when it is run
GRADIENTS = ("boundary", "discrete")                 # general.gradient: the reference's Hadamard formula (default) or the exact one


@dataclasses.dataclass
class OptimizationResults:
    compliance: list = dataclasses.field(default_factory=list)
    volume: list = dataclasses.field(default_factory=list)
    design_vector: list = dataclasses.field(default_factory=list)

    def append_result(self, design_vector, volume, compliance):
        self.volume.append(float(volume))
        self.compliance.append(float(compliance))
        self.design_vector.append(np.asarray(design_vector).tolist())


def _key(x):
    return str(np.asarray(x, dtype=np.float64).round(8))


class struct_optimization:
    """An optimisation folder holding ``config.json`` with the sections ``mesh`` (DeepSDFMesh's options), ``optimization``
    (``method`` and scipy's options, optional ``x0`` and ``bounds``) and ``general`` (``volume_constraint``; optional ``t_clamp``
    of the volume mesh, default 0; optional ``dense_dtheta``, default false; optional ``gradient``: "boundary" (default, the
    reference's Hadamard formula projected onto the normals) or "discrete" (the exact derivative of the discrete compliance and
    volume through the plain Jacobian; not with ``dense_dtheta``))."""

    def __init__(self, optimization_folder, experiment_location=None, device="cuda"):
        self.optimization_folder = pathlib.Path(optimization_folder)
        self.optimization_results = OptimizationResults()
        self.iteration = 0
        self.cache = {}
        self.device = device
        self.logger = logging.getLogger(__name__)
        if not self.settings_filename.exists():
            raise FileNotFoundError(f"{self.settings_filename} does not exist")
        self.load_settings()
        self.geometry = DeepSDFMesh(self.options["mesh"], experiment_location=experiment_location)
        self.problem = None

    @property
    def settings_filename(self):
        return self.optimization_folder / "config.json"

    @property
    def results_filename(self):
        return self.optimization_folder / "results.json"

    def load_settings(self):
        self.options = config.load_json(self.settings_filename)
        for key in ("mesh", "optimization", "general"):
            if key not in self.options:
                raise KeyError(f"config.json has no section {key!r}")
        method = self.options["optimization"]["method"]
        if method not in METHODS:
            raise ValueError(f"optimization.method {method!r} is not one of {list(METHODS)}")
        gradient = self.options["general"].get("gradient", "boundary")
        if gradient not in GRADIENTS:
            raise ValueError(f"general.gradient {gradient!r} is not one of {list(GRADIENTS)}")
        if gradient == "discrete" and bool(self.options["general"].get("dense_dtheta", False)):
            raise ValueError("general.gradient 'discrete' goes through the adjoint of the plain Jacobian: dense_dtheta (the dense, "
                             "clipped, normal-projected dTheta) cannot carry it")

    def set_x0(self):
        shape = (self.geometry.get_n_control_points(), self.geometry.get_latent_shape())
        x0 = np.zeros(shape)
        if "x0" in self.options["optimization"]:
            x0 = x0 + np.asarray(self.options["optimization"]["x0"], dtype=np.float64)
        self.start_values = x0.reshape(-1)
        self.dv_names = [f"x{i}" for i in range(self.start_values.size)]
        lb, ub = self.options["optimization"]["bounds"] if "bounds" in self.options["optimization"] else (-1, 1)
        self.bounds = [(lb, ub)] * self.start_values.size

    # ---- one evaluation ---------------------------------------------------------------------------------------------------------
    def _compute_solution(self, control_point_values):
        x = np.asarray(control_point_values, dtype=np.float64)
        self.iteration += 1
        general = self.options["general"]
        geo = self.geometry
        geo.generate_surface_mesh(x.reshape(-1, geo.get_latent_shape()))
        mesh = geo.generate_volume_mesh(t_clamp=float(general.get("t_clamp", 0.0)))
        beam = CantileverBeam(str(self.optimization_folder), device=self.device)
        beam.set_mesh(mesh)
        beam.set_up()
        dense = bool(general.get("dense_dtheta", False))
        discrete = general.get("gradient", "boundary") == "discrete"
        dTheta = geo.get_dTheta() if dense else None
        volume, der_vol = beam.compute_volume(dTheta)
        if not dense:
            der_vol = beam.compute_volume_gradient(geo, discrete=discrete)
        if np.any(np.isnan(der_vol)):
            self.logger.warning("the volume gradient holds a NaN")
        beam.solve()
        compliance, der_compliance = beam.compute_compliance(dTheta)
        if not dense:
            der_compliance = beam.compute_compliance_gradient(geo, discrete=discrete)
        self.problem = beam
        self.cache[_key(x)] = {"objective": (compliance, der_compliance),
                               "constraint": (volume - general["volume_constraint"], der_vol)}
        self.logger.debug(f"evaluation {self.iteration}: compliance {compliance}, volume {volume}")
        self.optimization_results.append_result(x, volume, compliance)
        with open(self.results_filename, "w") as fh:
            json.dump(dataclasses.asdict(self.optimization_results), fh)

    def _cached(self, x):
        if _key(x) not in self.cache:
            self._compute_solution(x)
        return self.cache[_key(x)]

    def objective(self, x):
        """(compliance, d compliance / d x [ncp * L])."""
        return self._cached(x)["objective"]

    def constraint(self, x):
        """(volume - volume_constraint, d volume / d x [ncp * L])."""
        return self._cached(x)["constraint"]

    # ---- drivers ----------------------------------------------------------------------------------------------------------------
    def run_optimization(self):
        self.logger.info(f"optimising in {self.optimization_folder} (pid {os.getpid()})")
        self.set_x0()
        method = self.options["optimization"]["method"]
        if method == "MMA":
            result = self.run_MMA_optimization(self.options["optimization"])
        else:
            result = self.run_scipy_optimization(self.options["optimization"])
        with open(self.results_filename, "w") as fh:
            json.dump(dataclasses.asdict(self.optimization_results), fh)
        return result

    def run_scipy_optimization(self, options):
        """scipy.optimize.minimize with the method config.json names; the remaining keys of ``optimization`` (but x0 and bounds)
        are its options.  BFGS takes the objective's gradient; COBYLA takes the values only, with the volume as an inequality
        (non-negative) constraint, as in the reference."""
        import scipy.optimize
        opts = {k: v for k, v in dict(options).items() if k not in ("method", "x0", "bounds")}
        method = options["method"]
        if method == "BFGS":                             # unconstrained and unbounded in scipy: value and gradient of the objective
            return scipy.optimize.minimize(lambda x: self.objective(x), self.start_values, jac=True, method=method, options=opts)
        cons = ({"type": "ineq", "fun": lambda x: self.constraint(x)[0]},)
        return scipy.optimize.minimize(lambda x: self.objective(x)[0], self.start_values, bounds=self.bounds, method=method,
                                       constraints=cons, options=opts)

    def run_MMA_optimization(self, options):
        raise NotImplementedError("method MMA needs the mmapy package (an MMA subproblem solver), which this package does not carry: "
                                  "use BFGS or COBYLA")
