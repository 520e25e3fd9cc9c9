"""ctypes binding of libdsdf_hip.so (include/dsdf.h).  Fails loudly when the library is missing: there is
no CPU fallback anywhere in this package."""
import ctypes as C
import os

import numpy as np
import torch  # before the library is loaded: lib() below says why

from .build import LIB

MAX_LAYERS = 16
ABI_VERSION = 19
MAX_BUCKETS = 8


class DsdfNet(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("latent_size", C.c_int32), ("geom_dim", C.c_int32),
                ("in_dim", C.c_int32 * MAX_LAYERS), ("out_dim", C.c_int32 * MAX_LAYERS),
                ("weight_norm_mask", C.c_uint32), ("dropout_mask", C.c_uint32), ("skip_mask", C.c_uint32),
                ("dropout_p", C.c_float), ("use_tanh", C.c_int32), ("fwd_bf16", C.c_int32),
                ("latent_dropout", C.c_int32), ("xyz_in_all", C.c_int32), ("ln_param_mask", C.c_uint32),
                ("gemm_split", C.c_int32)]


class DsdfParamLayout(C.Structure):
    _fields_ = [("total", C.c_int64), ("bias_off", C.c_int64 * MAX_LAYERS), ("g_off", C.c_int64 * MAX_LAYERS),
                ("v_off", C.c_int64 * MAX_LAYERS), ("ln_w_off", C.c_int64 * MAX_LAYERS), ("ln_b_off", C.c_int64 * MAX_LAYERS)]


class DsdfBatch(C.Structure):
    _fields_ = [("seg_scene", C.c_void_p), ("seg_offset", C.c_void_p), ("n_segments", C.c_int64),
                ("xyz", C.c_void_p), ("sdf_gt", C.c_void_p), ("n_points", C.c_int64), ("n_norm", C.c_int64),
                ("row_offset", C.c_int64), ("seg_len", C.c_int64)]


class DsdfLossCfg(C.Structure):
    _fields_ = [("clamp_dist", C.c_float), ("reg_coef", C.c_float), ("code_bound", C.c_float),
                ("training", C.c_int32), ("frozen_decoder", C.c_int32), ("dropout_key", C.c_uint32 * MAX_LAYERS),
                ("dw_phase", C.c_int32), ("dw_buckets", C.c_int32)]


class DsdfAdamCfg(C.Structure):
    _fields_ = [("step", C.c_int64), ("lr_decoder", C.c_float), ("lr_latent", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("eps", C.c_float), ("grad_scale", C.c_void_p)]


PROF_CLASSES = 8
PROF_NAMES = ("gemm_nt_kernel", "gemm_tn_kernel", "last_layer_kernel", "fused_forward_kernel", "fused_backward_kernel",
              "dw_stream_kernel", "other", "fused_fwd_bwd_kernel")


class DsdfProfile(C.Structure):
    _fields_ = [("ms", C.c_double * PROF_CLASSES), ("flops", C.c_double * PROF_CLASSES),
                ("count", C.c_int64 * PROF_CLASSES), ("dropped", C.c_int32)]


class DsdfMsGrid(C.Structure):
    _fields_ = [("dims", C.c_int32 * 3), ("tiling", C.c_int32 * 3)]


class DsdfMsSpline(C.Structure):
    _fields_ = [("degree", C.c_int32 * 3), ("n_cp", C.c_int32 * 3), ("n_knots", C.c_int32 * 3),
                ("knots_host", C.POINTER(C.c_float) * 3), ("knots_dev", C.c_void_p), ("cp", C.c_void_p), ("ncp", C.c_int64),
                ("L", C.c_int32)]


class DsdfMsCap(C.Structure):
    _fields_ = [("dim", C.c_int32), ("cap", C.c_int32), ("m", C.c_float), ("c", C.c_float)]


MS_MAX_CAPS = 6
MS_WEIGHTS = 64                        # weight slots per point of dsdf_ms_rows_at: (k * 4 + j) * 4 + i


class DsdfMsdMesh(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("edge_point", C.c_void_p), ("edge_axis", C.c_void_p), ("band_of", C.c_void_p),
                ("n_verts", C.c_int64), ("dims", C.c_int32 * 3), ("scale", C.c_float * 3), ("level", C.c_float)]


class DsdfMsdBand(C.Structure):
    _fields_ = [("G", C.c_void_p), ("weights", C.c_void_p), ("base", C.c_void_p), ("mask", C.c_void_p),
                ("n_band", C.c_int64), ("ld_g", C.c_int64), ("degree", C.c_int32 * 3), ("n_cp", C.c_int32 * 3),
                ("L", C.c_int32)]


class DsdfVdMesh(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("vert_point", C.c_void_p), ("vert_class", C.c_void_p), ("vert_index", C.c_void_p),
                ("band_of", C.c_void_p), ("n_verts", C.c_int64), ("n_moving", C.c_int64), ("dims", C.c_int32 * 3),
                ("scale", C.c_float * 3), ("level", C.c_float), ("t_clamp", C.c_float)]


class DsdfSgPlan(C.Structure):
    _fields_ = [("blocks", C.c_int32 * 3), ("n_blocks", C.c_int64), ("n_coarse", C.c_int64), ("n_points", C.c_int64),
                ("ws_bytes", C.c_size_t), ("state_offset", C.c_size_t), ("have_offset", C.c_size_t)]


class DsdfFemOp(C.Structure):
    _fields_ = [("tets", C.c_void_p), ("corner_order", C.c_void_p), ("vstart", C.c_void_p), ("geom", C.c_void_p),
                ("dinv", C.c_void_p), ("mask", C.c_void_p), ("n_verts", C.c_int64), ("n_tets", C.c_int64),
                ("lam", C.c_double), ("mu", C.c_double)]


class DsdfWsRegion(C.Structure):      # debug only: one row of dsdf_debug_ws_regions
    _fields_ = [("name", C.c_char * 24), ("offset", C.c_uint64), ("bytes", C.c_uint64)]


class DsdfPackedLayout(C.Structure):  # debug only: dsdf_debug_packed_layout
    _fields_ = [("total", C.c_int64), ("scale_off", C.c_int64)] + \
               [(k, C.c_int64 * MAX_LAYERS) for k in ("w_off", "wt_off", "wf_off", "wtf_off", "wfb_off", "ws_off", "wts_off",
                                                      "ws_plane", "wts_plane")] + \
               [(k, C.c_int32 * MAX_LAYERS) for k in ("ldw", "ldwt", "uf", "utf")]


WS_MAX_REGIONS = 192
WS_MAX_REDZONE = 4096
WS_PLAN_TRAIN, WS_PLAN_DECODE, WS_PLAN_DECODE_LATENT = 0, 1, 2
MEAN_WS_BYTES = 8192


class DsdfError(RuntimeError):
    pass


_P, _I64, _I32, _F, _SZ = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_size_t
_NET = C.POINTER(DsdfNet)
_D, _FEM = C.c_double, C.POINTER(DsdfFemOp)

# name -> argtypes; every function returns int except dsdf_last_error
PROTOTYPES = {
    "dsdf_abi_version": [],
    "dsdf_param_layout": [_NET, C.POINTER(DsdfParamLayout)],
    "dsdf_packed_floats": [_NET, C.POINTER(_I64)],
    "dsdf_workspace_bytes": [_NET, _I64, _I64, C.POINTER(_SZ)],
    "dsdf_decode_workspace_bytes": [_NET, _I64, C.POINTER(_SZ)],
    "dsdf_workspace_bytes_buckets": [_NET, _I64, _I64, _I32, C.POINTER(_SZ)],
    "dsdf_dw_phase_supported": [_NET],
    "dsdf_grad_buckets": [_NET, _I32, C.POINTER(_I32), C.POINTER(_I64)],
    "dsdf_materialize_weights": [_NET, _P, _P, _P],
    "dsdf_decode": [_NET, _P, _P, _P, _I64, _I64, _P, _P, _SZ, _P],
    "dsdf_module_forward": [_NET, _P, _P, _P, _I64, _I64, _I32, C.POINTER(C.c_uint32), _P, _P, _SZ, _P],
    "dsdf_module_backward": [_NET, _P, _P, _P, _I64, _I32, C.POINTER(C.c_uint32), _P, _I32, _P, _I64, _P, _SZ, _P],
    "dsdf_module_jvp": [_NET, _P, _P, _P, _I64, _I64, _I32, C.POINTER(C.c_uint32), _P, _P, _SZ, _P],
    "dsdf_train_forward_backward": [_NET, _P, _P, _P, _I64, C.POINTER(DsdfBatch), C.POINTER(DsdfLossCfg), _P, _P, _P,
                                    _P, _I32, _P, _SZ, _P],
    "dsdf_grad_norm": [_P, _I64, _F, _P, _P, _P, _SZ, _P],
    "dsdf_adam_step": [_NET, _P, _P, _P, _P, _P, _P, _P, _P, _I64, C.POINTER(DsdfAdamCfg), _P, _P],
    "dsdf_train_step": [_NET, _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, C.POINTER(DsdfBatch), C.POINTER(DsdfLossCfg),
                        C.POINTER(DsdfAdamCfg), _P, _P, _P, _SZ, _P],
    "dsdf_adam_latent_only": [_P, _P, _P, _P, _I64, C.POINTER(DsdfAdamCfg), _P],
    "dsdf_adam_latent_sched": [_P, _P, _P, _P, _I64, _P, _I64, _P, _F, _F, _F, _F, _P],
    "dsdf_profile_enable": [_I32],
    "dsdf_profile_read": [C.POINTER(DsdfProfile)],
    "dsdf_gemm_nt": [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _P],
    "dsdf_gemm_tn": [_P, _I64, _P, _I64, _P, _I64, _I64, _I64, _I64, _P, _SZ, _P],
    "dsdf_dropout_mask": [C.c_uint32, _F, _I64, _I64, _I64, _P, _P],
    "dsdf_decode_latent": [_NET, _P, _P, _P, _P, _I64, _P, _P, _SZ, _P],
    "dsdf_decode_latent_supported": [_NET],
    "dsdf_sample_batch": [_P, C.c_int32, _P, _P, _P, _P, _P, _I64, _I64, C.c_uint64, _P, _P, _P],
    "dsdf_sample_batch_seq": [_P, C.c_int32, _P, _P, _P, _P, _P, _I64, _I64, C.c_uint64, C.c_uint64, _P, _P, _P, _P],
    "dsdf_mc_workspace_bytes": [_I32, _I32, _I32, C.POINTER(_SZ)],
    "dsdf_mc_count": [_P, _I32, _I32, _I32, _F, _P, _P, _SZ, _P],
    "dsdf_mc_emit": [_P, _I32, _I32, _I32, _F, C.POINTER(_F), C.POINTER(_F), _I64, _I64, _P, _P, _P, _SZ, _P],
    "dsdf_mc_case_table": [_P, _SZ, C.POINTER(_I32)],
    "dsdf_msdf_plan": [_I64, _I64, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_I32)],
    "dsdf_msdf_prepare": [_P, _I64, _P, _I64, _P, _SZ, _P],
    "dsdf_ms_rows": [C.POINTER(DsdfMsSpline), C.POINTER(DsdfMsGrid), _I64, _I64, _P, _I32, _I32, _P, _P],
    "dsdf_ms_caps": [C.POINTER(DsdfMsGrid), _I64, _I64, C.POINTER(DsdfMsCap), _I32, _P, _P],
    "dsdf_debug_ws_redzone": [_I32],
    "dsdf_debug_ws_regions": [C.POINTER(DsdfWsRegion), _I32, C.POINTER(_I32), C.POINTER(_SZ)],
    "dsdf_debug_ws_plan": [_NET, _I64, _I64, _I32, _I32, _I32, _I32],
    "dsdf_debug_packed_layout": [_NET, C.POINTER(DsdfPackedLayout)],
    "dsdf_msdf_query": [_P, _I64, _P, _I64, _P, _P, _P, _P, _P, _I32, _P, _SZ, _P],
    "dsdf_module_input_grad": [_NET, _P, _P, _P, _I64, _P, _I64, _P, _SZ, _P],
    "dsdf_mc_edges": [_I32, _I32, _I32, _I64, _P, _P, _P, _SZ, _P],
    "dsdf_ms_rows_at": [C.POINTER(DsdfMsSpline), C.POINTER(DsdfMsGrid), _P, _I64, _P, _P, _P, _P],
    "dsdf_msd_vjp_workspace_bytes": [_I64, _I64, _I32, C.POINTER(_SZ), C.POINTER(_I32)],
    "dsdf_msd_jacobian": [C.POINTER(DsdfMsdMesh), C.POINTER(DsdfMsdBand), _I32, _P, _P, _P],
    "dsdf_msd_jvp": [C.POINTER(DsdfMsdMesh), C.POINTER(DsdfMsdBand), _P, _P, _P],
    "dsdf_msd_vjp": [C.POINTER(DsdfMsdMesh), C.POINTER(DsdfMsdBand), _P, _P, _P, _SZ, _P],
    "dsdf_vd_vjp_workspace_bytes": [_I64, _I64, _I32, C.POINTER(_SZ), C.POINTER(_I32)],
    "dsdf_vd_jvp": [C.POINTER(DsdfVdMesh), C.POINTER(DsdfMsdBand), _P, _P, _P],
    "dsdf_vd_vjp": [C.POINTER(DsdfVdMesh), C.POINTER(DsdfMsdBand), _P, _P, _P, _SZ, _P],
    "dsdf_vd_dtheta": [C.POINTER(DsdfVdMesh), C.POINTER(DsdfMsdBand), _P, C.POINTER(_F), _F, _P, _P],
    "dsdf_nn_plan": [_I64, _I64, C.POINTER(_SZ), C.POINTER(_I32)],
    "dsdf_nn_query": [_P, _I64, _P, _I64, _P, _P, _P, _SZ, _P],
    "dsdf_mean_f64": [_P, _I64, _P, _P, _SZ, _P],
    "dsdf_surf_plan": [_I64, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_I32)],
    "dsdf_surf_prepare": [_P, _I64, _P, _I64, _P, _SZ, C.POINTER(C.c_double), _P],
    "dsdf_surf_sample": [_P, _I64, _P, _I64, _P, _SZ, _I64, C.c_uint64, C.c_uint64, _F, _P, _P, _P, _P],
    "dsdf_mt_plan": [_I64, _I64, C.POINTER(_SZ)],
    "dsdf_mt_edge_keys": [_P, _I64, _I64, _P, _P],
    "dsdf_mt_adjacency": [_P, _I64, _P, _P, _P, _P, _P, _SZ, _P],
    "dsdf_mt_components": [_P, _I64, _P, _P, C.POINTER(_I32), _P, _SZ, _P],
    "dsdf_mt_face_degenerate": [_P, _I64, _P, _I64, _P, _P],
    "dsdf_mt_vertex_geometry": [_P, _I64, _P, _I64, _P, _P, _P, _P, _P],
    "dsdf_mt_volume": [_P, _I64, _P, _I64, _P, _P, _SZ, _P],
    "dsdf_mt_project": [_P, _P, _P, _I64, _I64, C.POINTER(_F), _F, _P, _P],
    "dsdf_sg_plan": [_I32, _I32, _I32, _I32, C.POINTER(DsdfSgPlan)],
    "dsdf_sg_coarse": [_I32, _I32, _I32, _I32, _P, _P, _SZ, _P],
    "dsdf_sg_seed": [_P, _I32, _I32, _I32, _I32, _F, _F, _P, _P, _SZ, _P],
    "dsdf_sg_grow": [_P, _I32, _I32, _I32, _I32, _F, _P, _P, _SZ, _P],
    "dsdf_sg_points_count": [_I32, _I32, _I32, _I32, _P, _P, _SZ, _P],
    "dsdf_sg_points_emit": [_I32, _I32, _I32, _I32, _I64, _P, _P, _SZ, _P],
    "dsdf_sg_fill": [_P, _I32, _I32, _I32, _I32, _P, _SZ, _P],
    "dsdf_sg_coords": [_I32, _I32, _I32, C.POINTER(_F), C.POINTER(_F), _P, _I64, _P, _P],
    "dsdf_sg_scatter": [_P, _I64, _P, _P, _I64, _P],
    "dsdf_sg_caps_at": [C.POINTER(DsdfMsGrid), _P, _I64, C.POINTER(DsdfMsCap), _I32, _P, _P],
    "dsdf_tet_workspace_bytes": [_I32, _I32, _I32, C.POINTER(_SZ)],
    "dsdf_tet_count": [_P, _I32, _I32, _I32, _F, _P, _P, _SZ, _P],
    "dsdf_tet_emit": [_P, _I32, _I32, _I32, _F, C.POINTER(_F), C.POINTER(_F), _F, _I64, _I64, _I64, _P, _P, _P, _P, _P, _P, _P, _SZ,
                      _P],
    "dsdf_tet_components": [_P, _I32, _I32, _I32, _F, _P, _P, C.POINTER(_I32), _P, _SZ, _P],
    "dsdf_fem_plan": [_I64, _I64, _I64, C.POINTER(_SZ)],
    "dsdf_fem_setup": [_FEM, _P, _P, _P, _P, _P, _SZ, _P],
    "dsdf_fem_apply": [_FEM, _P, _P, _P, _SZ, _P],
    "dsdf_fem_load": [_P, _I64, _P, _I64, _P, _P, _P, C.POINTER(_D), _P, _P, _P],
    "dsdf_fem_solve": [_FEM, _P, _P, _D, _I32, _I32, C.POINTER(_I32), C.POINTER(_I32), C.POINTER(_D), _P, _SZ, _P],
    "dsdf_fem_energy": [_FEM, _P, _P, _I32, _P, _P, _P, _SZ, _P],
    "dsdf_fem_boundary_gradient": [_P, _I64, _P, _I64, _P, _P, _P, _P, _P],
    "dsdf_fem_stiffness_gradient": [_FEM, _P, _P, _P, _P, _SZ, _P],
    "dsdf_fem_load_gradient": [_P, _I64, _P, _I64, _P, _P, _P, C.POINTER(_D), _P, _P, _P, _P],
}

_lib = None


def lib():
    """Load libdsdf_hip.so once.  Raises if it has not been built (python -m deepsdf_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch bundles its own libamdhip64; it must be in the process BEFORE our library is dlopen'ed so that both use
    # ONE HIP runtime (loaded the other way round, ours binds /opt/rocm's copy and sees "no ROCm-capable device"): the import
    # at the top of this module
    if not os.path.exists(LIB):
        raise DsdfError(f"{LIB} is missing: build it with `python -m deepsdf_amd.build` "
                        "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    h = C.CDLL(LIB)
    for name, args in PROTOTYPES.items():
        fn = getattr(h, name)  # AttributeError here = header/library mismatch
        fn.argtypes = args
        fn.restype = C.c_int
    h.dsdf_last_error.argtypes = []
    h.dsdf_last_error.restype = C.c_char_p
    v = h.dsdf_abi_version()
    if v != ABI_VERSION:
        raise DsdfError(f"libdsdf_hip.so ABI {v} != binding ABI {ABI_VERSION}: rebuild")
    _lib = h
    return h


def ws_regions():
    """Debug only: (rows, total) of the last workspace plan laid out on this thread (dsdf_debug_ws_regions);
    rows = [(name, offset, bytes)] in layout order."""
    n, total = C.c_int32(), C.c_size_t()
    table = (DsdfWsRegion * WS_MAX_REGIONS)()
    check(lib().dsdf_debug_ws_regions(table, WS_MAX_REGIONS, C.byref(n), C.byref(total)))
    return [(table[i].name.decode(), int(table[i].offset), int(table[i].bytes)) for i in range(n.value)], int(total.value)


def ptr(t):
    """A tensor's address for a void* argument; None is NULL."""
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    """torch's current stream for a `void* stream` argument."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def triple(x, what):
    """Three floats from a scalar or a sequence of three."""
    t = [float(v) for v in (x if isinstance(x, (list, tuple, np.ndarray, torch.Tensor)) else [x] * 3)]
    if len(t) != 3:
        raise ValueError(f"{what} needs 3 values, got {len(t)}")
    return t


def check(rc):
    if rc != 0:
        raise DsdfError(f"libdsdf_hip error {rc}: {lib().dsdf_last_error().decode()}")
