"""``analysis/geometry.py`` of the reference, its surface half, on the GPU.

``DeepSDFMesh`` takes the reference's option dictionary and gives the optimiser what it needs from the surface alone: a clean,
closed surface (deepsdf_amd.surface.SurfaceMesh), its vertex normals, the normal-projected shape derivative (``get_dTheta_surface``)
and the enclosed volume with its derivative with respect to the control points.  The volume mesh comes from the grid the surface
came from (``generate_volume_mesh``, ``export_mfem_mesh``: deepsdf_amd.tetmesh); the reference's route through tetgenpy and gustaf
is not part of this package: ``tetrahedralize_surface`` and ``export_volume_mesh`` raise NotImplementedError."""
import logging
import os
import pathlib

import numpy as np
import torch

from deepsdf_amd import workspace as ws
from deepsdf_amd.mesh import microstructure_mesh_diff, sdf_struct  # noqa: F401  (sdf_struct: re-exported)
from deepsdf_amd.spline import BSplineField
from deepsdf_amd.surface import SurfaceMesh
from deepsdf_amd.tetmesh import tetrahedralize

STRETCH = (2.0, 1.0, 1.0)      # the reference's "freeform deformation": x is doubled
CLIP = 1.0                     # its outlier rule: Jacobian entries outside [-1, 1] are zeroed


class DeepSDFMesh:
    """Generates a microstructure surface, and its derivatives, from a DeepSDF experiment."""

    def __init__(self, mesh_options, experiment_location=None):
        if "experiment_directory" not in mesh_options:
            raise KeyError("Key experiment_directory not found in general settings")
        if "checkpoint" not in mesh_options:
            raise KeyError("Key checkpoint not found in general settings")
        if not os.path.exists(mesh_options["experiment_directory"]):
            raise FileNotFoundError(f"Experiment directory {mesh_options['experiment_directory']} not found")
        self.options = mesh_options
        location = pathlib.Path("." if experiment_location is None else experiment_location)
        self.exp_dir = location / self.options["experiment_directory"]
        checkpoint = self.options["checkpoint"]
        latent = ws.load_latent_vectors(str(self.exp_dir), checkpoint)
        if isinstance(latent, list):
            latent = torch.stack([c.reshape(-1) for c in latent])
        self.latent = latent.to("cpu").numpy()
        self.decoder = ws.load_trained_model(str(self.exp_dir), checkpoint)
        self.decoder.eval()
        degrees = [int(p) for p in self.options["degrees"]]
        knots = [[-1.0] * (p + 1) + [1.0] * (p + 1) for p in degrees]
        n_initial = int(np.prod([p + 1 for p in degrees]))
        field = BSplineField(degrees, knots, np.zeros((n_initial, self.latent.shape[1])))      # zero codes at every control point
        field.uniform_refine(self.options["refinement"])
        self.latent_vec_interpolation = field
        self.surface_mesh = self.jacobian = self.diff = self.volume_mesh = self.volume_diff = None
        self.logger = logging.getLogger(__name__)
        self.logger.debug(f"Initialied latent vector with {field.control_mesh_resolutions} control points")

    def get_latent_shape(self) -> int:
        return self.latent.shape[1]

    def get_n_control_points(self) -> int:
        return self.latent_vec_interpolation.control_points.shape[0]

    def generate_surface_mesh(self, control_points):
        """Mesh and d vertices / d control points for these control points; x stretched by 2; then the reference's clean-up:
        the largest face-adjacency component when ``remove_orphans``, the watertightness test, and degenerate faces dropped when it
        fails.  Sets ``surface_mesh`` (a SurfaceMesh whose vertex ids are those of the derivative) and ``jacobian`` (the
        MicrostructureMeshDiff: its vjp / jvp / jacobian(), unstretched and unclipped; get_dTheta_surface applies both).

        Optional option keys ``sparse_block`` (cells per block edge) and ``sparse_lipschitz`` (default 1.0): decode only the blocks
        the surface passes through (deepsdf_amd.mesh.follow_surface).  Absent: the dense grid."""
        tiling = self.options["tiling"]
        N = [self.options["N_base_reconstruction"] * t + 1 for t in tiling]
        self.latent_vec_interpolation.control_points = control_points
        self.diff = microstructure_mesh_diff(tiling, self.decoder, self.latent_vec_interpolation, N,
                                             cap_border_dict=self.options["cap_border_dict"],
                                             block=self.options.get("sparse_block"),
                                             lipschitz=self.options.get("sparse_lipschitz", 1.0))
        mesh = SurfaceMesh.from_diff(self.diff, STRETCH)
        if self.options["remove_orphans"]:
            self.logger.debug("Removing orphan meshs")
            mesh = mesh.keep_largest_component()
        if not mesh.is_watertight:
            self.logger.debug("Mesh is not watertight - trying to fix by eliminating degenerate faces")
            mesh = mesh.drop_degenerate_faces()
            if not mesh.is_watertight:
                self.logger.warning("Mesh is still not watertight after eliminating degenerate faces")
            else:
                self.logger.debug("Successfully fixed mesh.")
        self.surface_mesh = mesh
        self.jacobian = self.diff

    def _mesh(self):
        if self.surface_mesh is None:
            raise RuntimeError("call generate_surface_mesh(control_points) first")
        return self.surface_mesh

    def get_dTheta_surface(self):
        """The reference's get_dTheta restricted to the surface vertices: [V, 3, ncp * L] fp32 on the device."""
        normals = self._mesh().vertex_normals()
        n_zero = int((normals == 0).all(1).sum())
        if n_zero > 0:
            self.logger.debug(f"{n_zero} 0-Normal vectors detected")
        return self._mesh().dtheta(clip=CLIP)

    def volume(self):
        return self._mesh().volume()

    def volume_gradient(self):
        """d volume / d control points [ncp, L] on the device."""
        return self._mesh().volume_gradient()

    def generate_volume_mesh(self, t_clamp=0.0):
        """The tetrahedral mesh of the solid the surface bounds, after generate_surface_mesh: the capped grid the surface came from
        (``diff.grid``) meshed at the voxel size, in the surface's coordinates ((v - voxel_size) / 2 in float64, x stretched by 2);
        only the largest solid component when ``remove_orphans``.  Sets and returns ``volume_mesh`` (a TetMesh); its axis-class
        boundary vertices are the surface's vertices bit for bit.  t_clamp: deepsdf_amd.tetmesh.tetrahedralize.  Also sets
        ``volume_diff`` (a deepsdf_amd.mesh.VolumeMeshDiff: the derivative of every moving vertex of the volume mesh, unstretched;
        get_dTheta and shape_gradient apply the stretch)."""
        self._mesh()
        vs = self.diff.voxel_size
        m = tetrahedralize(self.diff.grid, 0.0, vs, t_clamp=t_clamp, keep_largest=bool(self.options["remove_orphans"]),
                           return_edges=True)
        dev = m.verts.device
        verts = (m.verts.double() - torch.tensor(vs, dtype=torch.float64, device=dev)) / 2      # microstructure_mesh_diff's transform
        m.verts = verts * torch.tensor(STRETCH, dtype=torch.float64, device=dev)                 # SurfaceMesh.from_diff's stretch
        self.volume_mesh = m
        self.volume_diff = self.diff.for_tetmesh(m, t_clamp)
        return m

    def _volume(self):
        if self.volume_mesh is None or self.volume_diff is None:
            raise RuntimeError("call generate_volume_mesh() first")
        return self.volume_mesh, self.volume_diff

    def volume_normals(self):
        """[V_vol, 3] fp32: the vertex normals of the volume mesh's boundary (zero at interior vertices)."""
        return self._volume()[0].boundary_surface().vertex_normals()

    def get_dTheta(self):
        """The reference's get_dTheta (analysis/geometry.py:176-197) on the volume mesh: [V_vol, 3, ncp * L] fp32 on the device,
        every column of the Jacobian of every vertex stretched by STRETCH, entries outside [-CLIP, CLIP] zeroed, projected onto the
        vertex normal of ``volume_mesh.boundary_surface()``.  Rows of vertices that do not move (grid vertices, vertices the clamp
        holds) are zero.  Raises MemoryError, stating the size, when the array would not fit the device."""
        mesh, vd = self._volume()
        V, R = mesh.n_verts, vd.n_control_points * vd.latent_size
        need = 4 * V * 3 * R
        free = torch.cuda.mem_get_info(vd.device)[0]
        if need + 4 * vd.moving.numel() * 3 * R > free:
            raise MemoryError(f"dTheta [{V}, 3, {R}] fp32 takes {need} bytes ({need / 2 ** 30:.2f} GiB) besides the moving vertices' "
                              f"{4 * vd.moving.numel() * 3 * R}, the device has {free} bytes free: use shape_gradient, or a coarser grid")
        normals = self.volume_normals()
        n_zero = int((normals[vd.moving.long()] == 0).all(1).sum())
        if n_zero > 0:
            self.logger.debug(f"{n_zero} 0-Normal vectors detected")
        out = torch.zeros(V, 3, R, dtype=torch.float32, device=vd.device)
        out[vd.moving.long()] = vd.dtheta_moving(normals, STRETCH, CLIP)
        return out

    def shape_gradient(self, grad_verts, project=True):
        """grad_verts [V_vol, 3] -> [ncp, L] fp32 on the device: sum_v grad_verts[v] . dTheta[v, :, (k, l)] without the dense array.
        project=True: the adjoint of get_dTheta with clip = 0, i.e. the vjp of STRETCH * n (n . g) / (n . n); project=False: the
        adjoint of the plain stretched Jacobian, the vjp of STRETCH * g.  This path has NO outlier clipping: the reference's rule
        zeroes single entries of the dense Jacobian, which the adjoint never forms."""
        mesh, vd = self._volume()
        g = torch.as_tensor(grad_verts).to(vd.device, torch.float32)
        if g.shape != (mesh.n_verts, 3):
            raise ValueError(f"grad_verts must be [{mesh.n_verts}, 3], got {tuple(g.shape)}")
        if project:
            n = self.volume_normals()
            nn = (n * n).sum(1, keepdim=True)
            g = torch.where(nn > 0, n * ((n * g).sum(1, keepdim=True) / nn.clamp_min(1e-30)), torch.zeros_like(g))
        return vd.vjp(g * torch.tensor(STRETCH, dtype=torch.float32, device=vd.device))

    def export_mfem_mesh(self, filename):
        """Write ``volume_mesh`` as an MFEM mesh v1.0 file with the reference's boundary attributes (1: x = 0, 2: the top in z,
        3: the rest; TetMesh.boundary_attributes)."""
        if self.volume_mesh is None:
            raise RuntimeError("call generate_volume_mesh() first")
        self.volume_mesh.write_mfem(filename)

    def tetrahedralize_surface(self):
        """Not implemented (tetgenpy): generate_volume_mesh meshes the solid from the grid instead."""
        raise NotImplementedError("tetrahedralize_surface needs tetgenpy, which this package does not carry: only the surface stage "
                                  "(normals, volume, shape derivative) is implemented")

    def export_volume_mesh(self, filename, show_mesh=False, export_abaqus=False):
        """Not implemented (gustaf): export_mfem_mesh writes generate_volume_mesh's mesh."""
        raise NotImplementedError("export_volume_mesh needs a tetrahedral mesh (tetgenpy) and gustaf, which this package does not "
                                  "carry")


def transform(x, t):
    """The folding of an unfolded coordinate into one cell of a tiling of t cells (the fold of csrc/msgrid.hpp, in torch)."""
    period = 4.0 / t                                            # two cells: one and its mirror image
    return t * torch.abs(torch.remainder(x - t % 2, period) - period / 2) - 1
