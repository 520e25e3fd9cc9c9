"""P1 linear elasticity on a TetMesh (csrc/fem.hpp, dsdf_fem_*): what the reference does through mfem in
analysis/MFEMLinearElasticity.py, for order-1 tetrahedra and constant Lame coefficients, on the device the mesh already lives on.

    LinearElasticity(mesh, lam, mu)   element geometry, the matrix-free operator A = P K P + (I - P), its block-Jacobi preconditioner
        fix_faces / add_traction / add_nodal_forces     homogeneous Dirichlet faces and the load, by boundary attribute
        solve                                           preconditioned CG with MFEM's stopping rule; the scalars stay on the device
        work / compliance / strain_energy_density       f . u, u^T K u, w per element or per vertex
        compliance_shape_gradient / volume / volume_shape_gradient      per-vertex [V, 3] gradients of the Hadamard boundary formulas
        stiffness_gradient / load_gradient / compliance_discrete_gradient   the exact derivative of compliance() w.r.t. the vertices

fp64 throughout, no floating-point atomics, every sum in a fixed order: two runs give identical bytes.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

from . import _lib

NODAL = {"mean": 1, "last": 2}


def _corner_sort(ids, n_verts):
    """(order, vstart) of the corners ids.reshape(-1), stably sorted by vertex (SurfaceMesh._vertex_geometry's pair)."""
    corners, order = torch.sort(ids.reshape(-1).to(torch.int64), stable=True)
    vstart = torch.searchsorted(corners, torch.arange(n_verts + 1, dtype=torch.int64, device=ids.device))
    return order.contiguous(), vstart.contiguous()


class LinearElasticity:
    def __init__(self, mesh, lam, mu, attributes=None):
        if mesh.device.type != "cuda":
            raise _lib.DsdfError("LinearElasticity needs a mesh on a HIP device (no CPU fallback)")
        if mesh.n_verts < 1 or mesh.n_tets < 1:
            raise ValueError("LinearElasticity needs a mesh with at least one element")
        self.mesh, self.device = mesh, mesh.device
        self.lam, self.mu = float(lam), float(mu)
        self.nv, self.nt, self.nb = mesh.n_verts, mesh.n_tets, mesh.n_bfaces
        dev = self.device
        with torch.cuda.device(dev):
            self.verts = mesh.verts.to(torch.float64).contiguous()
            self.tets = mesh.tets.to(torch.int32).contiguous()
            self.bfaces = mesh.bfaces.to(torch.int32).contiguous()
            attr = mesh.boundary_attributes() if attributes is None else torch.as_tensor(attributes)
            self.attributes = attr.to(device=dev, dtype=torch.int32).reshape(-1)
            if self.attributes.shape[0] != self.nb:
                raise ValueError(f"attributes must have {self.nb} entries, got {self.attributes.shape[0]}")
            self.corder, self.vstart = _corner_sort(self.tets, self.nv)
            self.border, self.bvstart = _corner_sort(self.bfaces, self.nv)
            nb = C.c_size_t()
            _lib.check(_lib.lib().dsdf_fem_plan(self.nv, self.nt, self.nb, C.byref(nb)))
            self.ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
            self.geom = torch.empty(10, self.nt, dtype=torch.float64, device=dev)
            self.diag = torch.empty(self.nv, 6, dtype=torch.float64, device=dev)
            self.dinv = torch.empty(self.nv, 6, dtype=torch.float64, device=dev)
            self.mask = torch.empty(self.nv, dtype=torch.uint8, device=dev)
            self.fixed = torch.zeros(self.nv, dtype=torch.uint8, device=dev)
            self.f = torch.zeros(self.nv, 3, dtype=torch.float64, device=dev)
            self.u = torch.zeros(self.nv, 3, dtype=torch.float64, device=dev)
        self._n_fixed = 0
        self.tractions = []         # (selection [M] uint8, t): what add_traction summed into f, kept for load_gradient
        self.n_skipped_elements = self.n_held_vertices = None
        self._set_up()

    # ---- plumbing -------------------------------------------------------------------------------------------------------------
    def _op(self):
        return _lib.DsdfFemOp(self.tets.data_ptr(), self.corder.data_ptr(), self.vstart.data_ptr(), self.geom.data_ptr(),
                              self.dinv.data_ptr(), self.mask.data_ptr(), self.nv, self.nt, self.lam, self.mu)

    def _set_up(self):
        """Element geometry, preconditioner and mask for the current fixed set (again after every fix_faces)."""
        with torch.cuda.device(self.device):
            counts = torch.empty(2, dtype=torch.int64, device=self.device)
            op = self._op()
            _lib.check(_lib.lib().dsdf_fem_setup(C.byref(op), _lib.ptr(self.verts), _lib.ptr(self.fixed), _lib.ptr(self.diag), _lib.ptr(counts),
                                                 _lib.ptr(self.ws), self.ws.numel(), _lib.stream()))
            self.n_skipped_elements, self.n_held_vertices = counts.tolist()

    def _boundary_args(self):
        return (_lib.ptr(self.verts), self.nv, _lib.ptr(self.bfaces), self.nb, _lib.ptr(self.border), _lib.ptr(self.bvstart))

    def _vec(self, x, what):
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float64).contiguous()
        if x.shape != (self.nv, 3):
            raise ValueError(f"{what} must be [{self.nv}, 3], got {tuple(x.shape)}")
        return x

    # ---- the problem ----------------------------------------------------------------------------------------------------------
    def fix_faces(self, attr):
        """Clamp (u = 0) every vertex of the boundary triangles with this attribute: ess_bdr of CantileverBeam.set_up."""
        sel = self.attributes == int(attr)
        self._n_fixed += int(sel.sum())
        self.fixed[self.bfaces[sel].reshape(-1).long()] = 1
        self._set_up()              # diag, dinv, mask and the counts always describe the current fixed set
        return self

    def add_traction(self, attr, t):
        """Add the constant traction t (3 values) on the boundary triangles with this attribute: f_v += sum area_f / 3 * t."""
        t = [float(v) for v in t]
        if len(t) != 3:
            raise ValueError(f"a traction has 3 components, got {len(t)}")
        with torch.cuda.device(self.device):
            sel = (self.attributes == int(attr)).to(torch.uint8).contiguous()
            out = torch.empty(self.nv, 3, dtype=torch.float64, device=self.device)
            _lib.check(_lib.lib().dsdf_fem_load(*self._boundary_args(), _lib.ptr(sel), (C.c_double * 3)(*t), None, _lib.ptr(out), _lib.stream()))
            self.f += out
            self.tractions.append((sel, tuple(t)))
        return self

    def add_nodal_forces(self, f):
        self.f += self._vec(f, "nodal forces")
        return self

    def load(self):
        """P f [V, 3]: the load with the masked (fixed and held) vertices zeroed, as the solve uses it: selected, not multiplied, so
        that a value that is not finite at a masked vertex is dropped as fem_cg_start_kernel drops it."""
        return torch.where((self.mask != 0)[:, None], torch.zeros_like(self.f), self.f)

    def apply(self, x):
        """A x for x [V, 3]."""
        x = self._vec(x, "x")
        with torch.cuda.device(self.device):
            y = torch.empty_like(x)
            op = self._op()
            _lib.check(_lib.lib().dsdf_fem_apply(C.byref(op), _lib.ptr(x), _lib.ptr(y), _lib.ptr(self.ws), self.ws.numel(), _lib.stream()))
        return y

    def solve(self, rel_tol=1e-10, max_iter=10000, check_every=32):
        """(iterations, converged, <z, r> / <z0, r0>); the displacement is self.u [V, 3].  Neither depends on check_every."""
        if self._n_fixed == 0:
            raise ValueError("no fixed vertex: the operator is singular (call fix_faces with an attribute some boundary triangle carries)")
        it, conv, ratio = C.c_int32(), C.c_int32(), C.c_double()
        with torch.cuda.device(self.device):
            op = self._op()
            _lib.check(_lib.lib().dsdf_fem_solve(C.byref(op), _lib.ptr(self.f), _lib.ptr(self.u), float(rel_tol), int(max_iter), int(check_every),
                                                 C.byref(it), C.byref(conv), C.byref(ratio), _lib.ptr(self.ws), self.ws.numel(), _lib.stream()))
        return it.value, bool(conv.value), ratio.value

    # ---- after the solve ------------------------------------------------------------------------------------------------------
    def work(self):
        """f . u with the masked load, summed in fp64 in a fixed order."""
        return float((self.load() * self.u).sum(1).sum())

    def _energy(self, nodal, u=None):
        u = self.u if u is None else self._vec(u, "u")
        if nodal is not None and nodal not in NODAL:
            raise ValueError(f"nodal must be None, 'mean' or 'last', got {nodal!r}")
        with torch.cuda.device(self.device):
            we = torch.empty(self.nt, dtype=torch.float64, device=self.device)
            wv = torch.empty(self.nv, dtype=torch.float64, device=self.device) if nodal else None
            totals = torch.empty(2, dtype=torch.float64, device=self.device)
            op = self._op()
            _lib.check(_lib.lib().dsdf_fem_energy(C.byref(op), _lib.ptr(u), _lib.ptr(we), NODAL.get(nodal, 0), _lib.ptr(wv), _lib.ptr(totals),
                                                  _lib.ptr(self.ws), self.ws.numel(), _lib.stream()))
        return we, wv, totals

    def compliance(self):
        """sum V_e w_e = u^T K u: the reference's clcTotCompliance (sigma : eps, not half of it)."""
        return float(self._energy(None)[2][0])

    def strain_energy_density(self, nodal=None):
        """w per element [T] (nodal=None) or per vertex [V]: 'mean' the volume-weighted mean over the vertex's elements, 'last' the
        value of its element with the highest index (what mfem's ProjectCoefficient is believed to leave: unverified)."""
        we, wv, _ = self._energy(nodal)
        return we if nodal is None else wv

    def volume(self):
        return float(self._energy(None)[2][1])

    def _boundary_gradient(self, weight):
        with torch.cuda.device(self.device):
            g = torch.empty(self.nv, 3, dtype=torch.float64, device=self.device)
            _lib.check(_lib.lib().dsdf_fem_boundary_gradient(*self._boundary_args(), _lib.ptr(weight), _lib.ptr(g), _lib.stream()))
        return g

    def volume_shape_gradient(self):
        """gV [V, 3] = sum over the vertex's boundary triangles of A_f n_f / 3: clcVolumeShapeDerivative(theta) = sum gV . theta."""
        return self._boundary_gradient(None)

    def compliance_shape_gradient(self, nodal="mean"):
        """gC [V, 3] = -w_v sum A_f n_f / 3: clcComplianceShapeDerivative(theta) = sum gC . theta."""
        if nodal not in NODAL:
            raise ValueError(f"nodal must be 'mean' or 'last', got {nodal!r}")
        return self._boundary_gradient((-self._energy(nodal)[1]).contiguous())

    # ---- the exact discrete gradient ----------------------------------------------------------------------------
    def stiffness_gradient(self, u=None):
        """(gK [V, 3], emt [9, T]): gK_v = -sum over the vertex's corners of E_e g_a, E = V (w I - 2 H^T S) per element (nine exact
        zeros for a skipped one): the derivative of -u^T K(X) u with respect to the vertices at fixed u (default: the solved one)."""
        u = self.u if u is None else self._vec(u, "u")
        with torch.cuda.device(self.device):
            emt = torch.empty(9, self.nt, dtype=torch.float64, device=self.device)
            g = torch.empty(self.nv, 3, dtype=torch.float64, device=self.device)
            op = self._op()
            _lib.check(_lib.lib().dsdf_fem_stiffness_gradient(C.byref(op), _lib.ptr(u), _lib.ptr(emt), _lib.ptr(g), _lib.ptr(self.ws),
                                                              self.ws.numel(), _lib.stream()))
        return g, emt

    def load_gradient(self, u=None):
        """gL [V, 3], summed over the tractions in the order they were added: the derivative of f(X) . u with respect to the vertices
        at fixed u, the loaded faces' areas moving with the mesh.  Nodal forces are constants and add nothing."""
        u = self.u if u is None else self._vec(u, "u")
        with torch.cuda.device(self.device):
            total = torch.zeros(self.nv, 3, dtype=torch.float64, device=self.device)
            g = torch.empty_like(total)
            for sel, t in self.tractions:
                _lib.check(_lib.lib().dsdf_fem_load_gradient(*self._boundary_args(), _lib.ptr(sel), (C.c_double * 3)(*t), _lib.ptr(self.mask),
                                                             _lib.ptr(u), _lib.ptr(g), _lib.stream()))
                total += g
        return total

    def compliance_discrete_gradient(self):
        """gC [V, 3] = gK + 2 gL for the solved u: the derivative of the number compliance() returns with respect to the vertices,
        exact for the discrete problem (Pi = 2 f . u - u^T K u is stationary in the free components of u: no new solve)."""
        return self.stiffness_gradient()[0] + 2.0 * self.load_gradient()
