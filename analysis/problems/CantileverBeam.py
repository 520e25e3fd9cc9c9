"""The reference's ``analysis/problems/CantileverBeam.py`` on the GPU solver (deepsdf_amd.fem.LinearElasticity): the
same methods and return shapes, with no mfem behind them.  ``set_mesh`` is new: the route from ``DeepSDFMesh.generate_volume_mesh``
with no file in between."""
import numpy as np
import torch

from deepsdf_amd.fem import LinearElasticity
from deepsdf_amd.tetmesh import TetMesh

LAMBDA, MU = 0.0, 105.0                  # the reference's set_up
TRACTION = (0.0, 0.0, -0.01)
CLAMPED_ATTRIBUTE, LOADED_ATTRIBUTE = 1, 2


class CantileverBeam:
    def __init__(self, simulation_folder, device="cuda"):
        self.strain_energy_density_data = None
        self.u_data = None
        self.simulation_folder = simulation_folder
        self.device = device
        self.mesh = self.attributes = self.ElasticitySolver = None

    def read_mesh(self, mesh_filename):
        """An MFEM mesh v1.0 file of tetrahedra and boundary triangles (TetMesh.write_mfem's); its boundary attributes are kept."""
        mesh, attributes = TetMesh.read_mfem(mesh_filename)
        self.set_mesh(mesh, attributes)

    def set_mesh(self, tet_mesh, attributes=None):
        """A TetMesh (moved to the device); attributes [M]: default the reference's rule, tet_mesh.boundary_attributes()."""
        self.mesh = tet_mesh.to(self.device)
        self.attributes = self.mesh.boundary_attributes() if attributes is None else torch.as_tensor(attributes).to(self.mesh.device)
        self.ElasticitySolver = None
        self.u_data = self.strain_energy_density_data = None

    def show_mesh(self):
        raise NotImplementedError("show_mesh needs gustaf (gus.Volumes / gus.show), which this package does not depend on")

    def set_up(self, ref_levels=0, order=1):
        if ref_levels != 0:
            raise NotImplementedError("uniform refinement (ref_levels > 0) is not implemented: mesh at the resolution wanted")
        if order != 1:
            raise NotImplementedError("only order 1 (P1 tetrahedra) is implemented")
        if self.mesh is None:
            raise ValueError("No mesh found. Call read_mesh or set_mesh first.")
        s = LinearElasticity(self.mesh, LAMBDA, MU, attributes=self.attributes)
        s.fix_faces(CLAMPED_ATTRIBUTE)
        s.add_traction(LOADED_ATTRIBUTE, TRACTION)
        self.ElasticitySolver = s

    def solve(self, rel_tol=1e-10, max_iter=10000):
        """Solves the state; u_data is the displacement in mfem's by-component order (reshape(-1, 3, order="F") gives [V, 3]).
        Returns (iterations, converged, relative <z, r>).  The reference also writes a ParaView collection; this does not."""
        out = self.ElasticitySolver.solve(rel_tol=rel_tol, max_iter=max_iter)
        self.u_data = self.ElasticitySolver.u.cpu().numpy().reshape(-1, order="F")
        return out

    def save_paraview(self):
        raise NotImplementedError("ParaView output needs mfem.ParaViewDataCollection (or a VTK writer), which this package does not depend on")

    def show_solution(self, output, **kwargs):
        raise NotImplementedError("show_solution needs gustaf (gus.Volumes / gus.show), which this package does not depend on")

    def _contract(self, grad, dTheta):
        """sum_v grad_v . dTheta[v, :, k] for every k: [R] fp64 (the reference loops over k and assembles a linear form for each).  A
        product and torch's sum, not a BLAS call: the same bytes every time."""
        d = torch.as_tensor(dTheta).to(device=grad.device, dtype=torch.float64)
        if d.dim() != 3 or d.shape[:2] != grad.shape:
            raise ValueError(f"dTheta must be [{grad.shape[0]}, 3, R], got {tuple(d.shape)}")
        return (grad[:, :, None] * d).sum((0, 1)).cpu().numpy()

    def compute_shape_derivative(self):
        raise NotImplementedError("the reference calls clcShapeDerivative, which its solver does not define; use compute_compliance(dTheta)")

    def compute_compliance(self, dTheta=None, nodal="mean"):
        """(total compliance, derivative [R] for dTheta [V, 3, R] or array(None)): the reference's return shapes."""
        if self.u_data is None:
            raise ValueError("No solution found. Compute solution first to get Compliance.")
        s = self.ElasticitySolver
        self.strain_energy_density_data = s.strain_energy_density(nodal).cpu().numpy()
        compl_der = None if dTheta is None else self._contract(s.compliance_shape_gradient(nodal), dTheta)
        return s.compliance(), np.array(compl_der)

    def compute_volume(self, dTheta=None):
        if self.ElasticitySolver is None:
            raise ValueError("No solver found. Call set_up first.")
        s = self.ElasticitySolver
        vol_der = None if dTheta is None else self._contract(s.volume_shape_gradient(), dTheta)
        return s.volume(), np.array(vol_der)

    def compute_volume_gradient(self, geometry, discrete=False):
        """d volume / d control points [ncp * L] fp64 through ``geometry.shape_gradient`` (a DeepSDFMesh whose volume_mesh is this
        problem's mesh): the adjoint of compute_volume(dTheta)[1] with dTheta = geometry.get_dTheta(), without the dense array and
        without its outlier clipping.  discrete=True: the same vertex gradient (it is the exact derivative of the volume already)
        through the plain Jacobian, not projected onto the normals."""
        if self.ElasticitySolver is None:
            raise ValueError("No solver found. Call set_up first.")
        g = geometry.shape_gradient(self.ElasticitySolver.volume_shape_gradient(), project=not discrete)
        return g.double().reshape(-1).cpu().numpy()

    def compute_compliance_gradient(self, geometry, nodal="mean", discrete=False):
        """d compliance / d control points [ncp * L] fp64, the adjoint counterpart of compute_compliance(dTheta)[1].  discrete=True:
        the exact derivative of the discrete compliance (LinearElasticity.compliance_discrete_gradient) through the plain Jacobian;
        an exact vertex gradient has tangential parts that count, so it is not projected onto the normals (``nodal`` plays no part)."""
        if self.u_data is None:
            raise ValueError("No solution found. Compute solution first to get Compliance.")
        s = self.ElasticitySolver
        if discrete:
            g = geometry.shape_gradient(s.compliance_discrete_gradient(), project=False)
        else:
            g = geometry.shape_gradient(s.compliance_shape_gradient(nodal))
        return g.double().reshape(-1).cpu().numpy()
