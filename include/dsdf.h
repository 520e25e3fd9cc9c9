/* dsdf.h -- C ABI of libdsdf_hip.so: the DeepSDF auto-decoder training step on MI355X (gfx950).
 *
 * The reference (mkofler96/DeepSDF) has NO C/FFI boundary for this path: its hot loop is inline Python
 * (train_deep_sdf.py:481-545) over torch ops.  This header is therefore the boundary that a binding of
 * that loop would target; every entry point names the reference lines it replaces.  The Python side of
 * this repo (deepsdf_amd/_lib.py) binds it with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error (DSDF_E_*); dsdf_last_error() returns a
 *     thread-local message.  Nothing throws, nothing allocates device memory, nothing synchronises the
 *     device: work is enqueued on the caller's stream (hipStream_t passed as void*).
 *   - every pointer is a DEVICE pointer owned by the caller (a torch tensor kept alive by the caller),
 *     16-byte aligned, unless marked [host].
 *   - all tensors are row-major fp32; index arrays are int64.
 *   - decoder parameters, their gradients and Adam moments live in flat "arenas" whose layout is the
 *     reference module's named_parameters() order (dsdf_param_layout).
 */
#ifndef DSDF_H
#define DSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSDF_MAX_LAYERS 16
#define DSDF_ABI_VERSION 19
#define DSDF_MAX_BUCKETS 8

enum {
  DSDF_OK = 0,
  DSDF_E_INVALID = -1,   /* bad argument (shape, alignment, unsupported NetworkSpecs variant) */
  DSDF_E_WORKSPACE = -2, /* workspace too small */
  DSDF_E_LAUNCH = -3     /* a HIP call failed */
};

/* Architecture of deep_sdf/networks/deep_sdf_decoder.py:10-73 after its layer-size arithmetic (:29-48).
 * Layer l is Linear(in_dim[l] -> out_dim[l]); hidden layers apply ReLU (+dropout); the last layer
 * (out_dim == 1) is followed by tanh (twice if use_tanh), :94-95,108-109. */
typedef struct DsdfNet {
  int32_t n_layers;                 /* number of Linear layers (= len(dims)+1) */
  int32_t latent_size;              /* L  (CodeLength) */
  int32_t geom_dim;                 /* G  (geom_dimension) */
  int32_t in_dim[DSDF_MAX_LAYERS];
  int32_t out_dim[DSDF_MAX_LAYERS];
  uint32_t weight_norm_mask;        /* bit l: layer l is weight-normed (g = original0, v = original1) */
  uint32_t dropout_mask;            /* bit l: F.dropout after layer l's ReLU (:105-106) */
  uint32_t skip_mask;               /* bit l: layer l's input is [x || x0]  (latent_in, :88-89) */
  float dropout_p;
  int32_t use_tanh;
  int32_t fwd_bf16;                 /* BASELINE config 5: hidden-layer forward GEMMs take bf16 inputs (weights and layer inputs
                                       rounded to nearest-even), fp32 accumulate on v_mfma_f32_32x32x16_bf16; the output layer,
                                       the backward pass, master weights and Adam stay fp32.  Needs every width <= 512. */
  /* Decoder variants no shipped spec uses (layer-by-layer kernels, general mode; not with fwd_bf16): */
  int32_t latent_dropout;           /* deep_sdf_decoder.py:79-82: in training, layer 0 sees F.dropout(latent, 0.2) (the skip layer
                                       still concatenates the original input); mask = the dropout hash under dropout_key[15] */
  int32_t xyz_in_all;               /* :90-91: every layer l >= 1 that is not a latent_in layer takes [x || xyz]
                                       (in_dim[l] = out_dim[l-1] + geom_dim) */
  uint32_t ln_param_mask;           /* :60-65 (norm_layers WITHOUT weight_norm): bit l: a bn{l} = nn.LayerNorm(out_dim[l]) module exists
                                       (parameters bn{l}.weight, bn{l}.bias right after lin{l}.weight, lin{l}.bias); forward applies it
                                       between the Linear and the ReLU of every HIDDEN layer that has one (:97-103) */
  int32_t gemm_split;               /* opt-in: the hidden-layer GEMMs of the three MFMA-bound kernels (forward, backward dX chain, dW) run on the bf16 matrix
                                       pipe with every fp32 operand cut into three bf16 terms (6 of the 9 cross products, fp32 accumulate):
                                       fp32 accuracy (same parity tolerances), 2.7 x the MFMA rate.  Needs every width <= 512; not with the
                                       variants above.  Together with fwd_bf16: the bf16 forward as it is, the backward dX chain in split
                                       and dW in split mode.  Everything else is unchanged. */
} DsdfNet;

/* Offsets (in floats) of every parameter tensor inside the decoder arena, named_parameters() order:
 * weight-normed layer: bias, g [out,1], v [out,in];  plain layer: weight [out,in], bias. */
typedef struct DsdfParamLayout {
  int64_t total;
  int64_t bias_off[DSDF_MAX_LAYERS];
  int64_t g_off[DSDF_MAX_LAYERS];   /* -1 for plain layers */
  int64_t v_off[DSDF_MAX_LAYERS];   /* v (weight-normed) or weight (plain) */
  int64_t ln_w_off[DSDF_MAX_LAYERS]; /* bn{l}.weight (LayerNorm gamma), -1 if layer l has no bn module */
  int64_t ln_b_off[DSDF_MAX_LAYERS]; /* bn{l}.bias   (LayerNorm beta) */
} DsdfParamLayout;

/* Batch of one optimiser (sub-)step, train_deep_sdf.py:483-501.  Points are grouped in R contiguous
 * runs ("segments"), run r = points [seg_offset[r], seg_offset[r+1]) all of scene seg_scene[r]; this is
 * the layout `indices.unsqueeze(-1).repeat(1, S)` (+ torch.chunk) always produces. */
typedef struct DsdfBatch {
  const int64_t* seg_scene;   /* [R]   row of the latent table */
  const int64_t* seg_offset;  /* [R+1] seg_offset[0] = 0, seg_offset[R] = n_points */
  int64_t n_segments;         /* R */
  const float* xyz;           /* [n_points, G] */
  const float* sdf_gt;        /* [n_points]  (unclamped; clamped inside, :493) or NULL for inference */
  int64_t n_points;           /* N of this chunk */
  int64_t n_norm;             /* loss normaliser: the FULL step's point count, also across ranks (:519) */
  int64_t row_offset;         /* index of this chunk's first point inside the step (dropout hash) */
  int64_t seg_len;            /* > 0: EVERY segment has exactly this many points (the reference's B x S layout, also per
                                 --batch_split chunk when chunks hold whole scenes); 0: irregular.  A multiple of 64
                                 selects SEGMENT MODE: the per-scene latent products are computed once per scene instead
                                 of once per point (same results up to fp32 summation order). */
} DsdfBatch;

typedef struct DsdfLossCfg {
  float clamp_dist;           /* ClampingDistance delta (:335,493,517) */
  float reg_coef;             /* CodeRegularizationLambda * min(1, epoch/100), 0 disables (:523-527) */
  float code_bound;           /* CodeBound (Embedding max_norm, :343,385); <= 0 disables the renorm */
  int32_t training;           /* 1: dropout active (decoder.train(), :477) */
  int32_t frozen_decoder;     /* 1: skip the decoder's weight gradients (latent-only optimisation, config 4); grads untouched */
  uint32_t dropout_key[DSDF_MAX_LAYERS]; /* [host-computed] per-layer hash keys (oracle: dropout_layer_key) */
  int32_t dw_phase;           /* data-parallel steps that exchange the decoder gradient in K = dw_buckets >= 2 buckets (replaces
                                 nn.DataParallel's reduce, train_deep_sdf.py:353), one call per bucket: 0 = the whole backward in this call
                                 (dw_buckets <= 1); 1 = everything except the weight gradients of the layers below bucket 0 -- on
                                 return (stream order) the arena holds the gradients of bucket 0 (the LAST layers), whose all-reduce
                                 can start; p in 2..K = only the weight gradients of bucket p - 1, from the activations / dP the
                                 phase-1 call left in `ws` (same net, batch, workspace and dw_buckets; nothing else may touch `ws` in
                                 between).  Buckets and their arena ranges: dsdf_grad_buckets.  Phases need the fused kernels
                                 (dsdf_dw_phase_supported), a trainable decoder and accumulate = 0. */
  int32_t dw_buckets;         /* K of dw_phase (0 or 1: no buckets); workspace: dsdf_workspace_bytes_buckets when K > 2 */
} DsdfLossCfg;

typedef struct DsdfAdamCfg {
  int64_t step;               /* 1-based, shared by every tensor (torch/optim/adam.py) */
  float lr_decoder, lr_latent;/* LearningRateSchedule[0], [1] at this epoch (:315-318) */
  float beta1, beta2, eps;    /* torch defaults 0.9, 0.999, 1e-8 (:400) */
  const float* grad_scale;    /* optional device scalar multiplying decoder grads (grad clipping), or NULL */
} DsdfAdamCfg;

/* ---- introspection ------------------------------------------------------------------------------ */
int dsdf_abi_version(void);
const char* dsdf_last_error(void);
int dsdf_param_layout(const DsdfNet* net, DsdfParamLayout* out);          /* [host] */
int dsdf_packed_floats(const DsdfNet* net, int64_t* n_floats);            /* [host] size of the packed-weight buffer */
int dsdf_workspace_bytes(const DsdfNet* net, int64_t n_points, int64_t n_segments, size_t* bytes); /* [host] train/module */
int dsdf_decode_workspace_bytes(const DsdfNet* net, int64_t n_points, size_t* bytes);                /* [host] dsdf_decode */

/* [host] workspace of a step that runs its backward in n_buckets phases (DsdfLossCfg.dw_buckets): the split-K slabs of a
 * bucket's weight-gradient launch are finer than the whole launch's.  dsdf_workspace_bytes covers n_buckets <= 2. */
int dsdf_workspace_bytes_buckets(const DsdfNet* net, int64_t n_points, int64_t n_segments, int32_t n_buckets, size_t* bytes);

/* ---- debug only: red zones and the region table of the workspace planners -------------------------------
 * Every entry point that takes `void* ws` cuts that one allocation into adjacent regions (layer inputs, dP buffers, masks,
 * column sums, split-K slabs, head partials, ...), each rounded up to 256 bytes.  These two entries let a TEST see a write that
 * leaves its region: it asks for red zones, fills the whole workspace with one byte value, runs a call, reads the layout the
 * call used and compares every byte outside the regions (red zones, rounding padding, the tail) with the fill value.  No
 * kernel takes part; production callers never call either entry.
 *
 * dsdf_debug_ws_redzone  [host] process-wide: every region of every planner (training / module, decode, decode_latent,
 *   marching cubes, mesh SDF, gemm_tn, grad_norm) is followed by `bytes` unused bytes.  0 (the default) or a multiple of
 *   256, at most DSDF_WS_MAX_REDZONE; anything else is DSDF_E_INVALID and changes nothing.  Every *_workspace_bytes /
 *   dsdf_msdf_plan answer and every entry point's size check include the red zones.  With 0 every offset and every total is
 *   exactly what it is without this mechanism.  Set it while no call is in flight, and size the workspace AFTER setting it.
 * dsdf_debug_ws_regions  [host] the layout of the LAST plan laid out on the calling thread: by a launching entry point (each
 *   records the plan it launched with), by dsdf_mc_workspace_bytes / dsdf_msdf_plan, or by dsdf_debug_ws_plan.  One row per
 *   region in layout order: `bytes` is the exact, unrounded size the planner asked for (deliberate over-read slack is part of
 *   the region that owns it); buffers that alias on purpose (inference ping-pong, the shared LayerNorm scratch) appear once.
 *   *n_regions and *total (the plan's size, red zones included; may be NULL) are always written.  table == NULL: only those
 *   two.  capacity < *n_regions: DSDF_E_INVALID, nothing written to table.  DSDF_WS_MAX_REGIONS rows always suffice.
 * dsdf_debug_ws_plan     [host] lays out the plan a launch WOULD use, without a launch or a device, and makes it the calling
 *   thread's last plan: kind DSDF_WS_PLAN_TRAIN (training step and the module path: n_segments, segmode, n_buckets, frows as
 *   the step chooses them -- dsdf_workspace_bytes answers the largest of these over segmode 0 / 1 and frows 32 / 64),
 *   DSDF_WS_PLAN_DECODE (dsdf_decode) or DSDF_WS_PLAN_DECODE_LATENT (dsdf_decode_latent); the latter two ignore n_segments,
 *   segmode and n_buckets.  frows is 32 or 64. */
#define DSDF_WS_MAX_REGIONS 192
#define DSDF_WS_MAX_REDZONE 4096
enum { DSDF_WS_PLAN_TRAIN = 0, DSDF_WS_PLAN_DECODE = 1, DSDF_WS_PLAN_DECODE_LATENT = 2 };
typedef struct DsdfWsRegion {
  char name[24];                    /* NUL-terminated: "in3", "part", "dwslab5", "mc_vbase", ... */
  uint64_t offset;                  /* bytes from the workspace pointer; a multiple of 256 */
  uint64_t bytes;                   /* exact size asked for (not rounded, red zone not included) */
} DsdfWsRegion;
int dsdf_debug_ws_redzone(int32_t bytes);
int dsdf_debug_ws_regions(DsdfWsRegion* table, int32_t capacity, int32_t* n_regions, size_t* total);
int dsdf_debug_ws_plan(const DsdfNet* net, int64_t n_points, int64_t n_segments, int32_t kind, int32_t segmode, int32_t n_buckets,
                       int32_t frows);

/* ---- debug only: where everything lies inside the packed-weight buffer ----------------------------------------------
 * dsdf_debug_packed_layout [host] the layout dsdf_materialize_weights / dsdf_adam_step / dsdf_train_step write `packed` with, so
 * that a TEST can state what every byte of the buffer must be.  No kernel takes part; production callers never call it.
 * Offsets are in floats from the start of `packed`; entries of layers >= n_layers are -1 (offsets) or 0.  Per layer l
 * (out x in = out_dim[l] x in_dim[l]; W = v * scale[row], scale = g / ||v_row|| or 1):
 *   w_off / ldw     W   [out][ldw]  row-major, ldw  = in  rounded up to 32
 *   wt_off / ldwt   W^T [in][ldwt]  row-major, ldwt = out rounded up to 32           (not written for the last layer)
 *   wf_off / uf     fragment order of B = W   (n = out, k = in ), uf  k-units of 16 per 32-row n-tile:
 *   wtf_off / utf   fragment order of B = W^T (n = in,  k = out), utf k-units:
 *                     Bf[((nt * U + u) * 2 + i) * 256 + lane * 4 + e] = B[32 nt + (lane & 31)][16 u + 8 (lane >> 5) + 4 i + e]
 *   wfb_off         fwd_bf16: bf16(W), round to nearest even, 32 k-unit slots of 512 bf16 per n-tile, unit u in slot
 *                     16 ((u >> 1) & 1) + 2 (u >> 2) + (u & 1); element ((nt * 32 + slot) * 64 + lane) * 8 + j (j = 4 i + e)
 *   ws_off / ws_plane, wts_off / wts_plane   gemm_split: W / W^T as three bf16 planes of `plane` bf16 elements each (x = h + m + l,
 *                     every term the top 16 bits of what is left), element ((nt * U + u) * 64 + lane) * 8 + j inside a plane
 * The fragment copies exist for every layer but the last; entries of an absent copy (last layer, flag not set) still carry the
 * offset the layout reserves for them.  Everything the kernels never write (leading-dimension padding, rows and k-units past the
 * matrix, n-tiles of the rounding to 4, unused slots) stays as the caller initialised it: the kernels rely on zeros there.
 * scale_off: one float per output row of every layer, layers in order.  total == dsdf_packed_floats. */
typedef struct DsdfPackedLayout {
  int64_t total, scale_off;
  int64_t w_off[DSDF_MAX_LAYERS], wt_off[DSDF_MAX_LAYERS], wf_off[DSDF_MAX_LAYERS], wtf_off[DSDF_MAX_LAYERS], wfb_off[DSDF_MAX_LAYERS];
  int64_t ws_off[DSDF_MAX_LAYERS], wts_off[DSDF_MAX_LAYERS], ws_plane[DSDF_MAX_LAYERS], wts_plane[DSDF_MAX_LAYERS];
  int32_t ldw[DSDF_MAX_LAYERS], ldwt[DSDF_MAX_LAYERS], uf[DSDF_MAX_LAYERS], utf[DSDF_MAX_LAYERS];
} DsdfPackedLayout;
int dsdf_debug_packed_layout(const DsdfNet* net, DsdfPackedLayout* out);

/* [host] 1 if this net's training step can run its backward in phases (the fused kernels take it; in this process: the
 * DSDF_NO_FUSED switch counts), 0 if not (a caller then exchanges the gradient in ONE piece), < 0 for an invalid net. */
int dsdf_dw_phase_supported(const DsdfNet* net);

/* [host] the K = n_buckets (2..DSDF_MAX_BUCKETS) gradient buckets of DsdfLossCfg.dw_phase, in the order the backward
 * finishes them (last layers first): bucket b = layers [first_layer[b], first_layer[b - 1]) (b = 0: up to the last layer)
 * = arena floats [arena_off[b + 1], arena_off[b]); arena_off has K + 1 entries, arena_off[0] = total, arena_off[K] = 0.
 * A net with fewer layers than buckets leaves trailing buckets empty. */
int dsdf_grad_buckets(const DsdfNet* net, int32_t n_buckets, int32_t* first_layer, int64_t* arena_off);

/* ---- weights -------------------------------------------------------------------------------------
 * W = g * v / ||v||_row for weight-normed layers (torch._weight_norm via parametrizations.weight_norm,
 * deep_sdf_decoder.py:50-55), plain copy otherwise; written as W [out,in] and W^T [in,out] in padded,
 * MFMA-friendly layouts (row-major W and W^T, plus fragment-ordered copies for the fused kernels).  `packed` must be
 * ZERO-INITIALISED once by the caller (padding tiles are never written).  Must be called after every parameter
 * change (dsdf_adam_step does it itself). */
int dsdf_materialize_weights(const DsdfNet* net, const float* params, float* packed, void* stream);

/* ---- inference: deep_sdf/utils.py:54-65 decode_sdf / Decoder.forward in eval mode ------------------
 * input [n, L+G] (latent first, xyz last) with row stride ld_in floats -> sdf [n]. */
int dsdf_decode(const DsdfNet* net, const float* packed, const float* params, const float* input, int64_t ld_in,
                int64_t n, float* sdf_out, void* ws, size_t ws_bytes, void* stream);

/* deep_sdf/utils.py:54-65 decode_sdf with ONE latent vector for all query points (what every caller does: mesh.py:61-70,
 * 262-271): sdf = Decoder.eval()([latent.expand(n) || xyz]).  The [n, L+G] input is never built: W[:, latent] latent is
 * computed once and enters the forward as the accumulators' initial value (segment mode).  latent [L],
 * xyz [n, G], sdf_out [n]; workspace: dsdf_decode_workspace_bytes.  Needs the fp32 fused forward (widths <= 512,
 * geom_dim <= 4, at least two hidden layers), otherwise DSDF_E_INVALID: use dsdf_decode. */
int dsdf_decode_latent(const DsdfNet* net, const float* packed, const float* params, const float* latent, const float* xyz,
                       int64_t n, float* sdf_out, void* ws, size_t ws_bytes, void* stream);
/* [host] 1 if dsdf_decode_latent accepts this net (in this process: the DSDF_NO_FUSED switch counts), 0 if the caller has
 * to build the [n, L+G] input and use dsdf_decode (variants on the layer-by-layer kernels: xyz_in_all, latent_dropout,
 * LayerNorm; widths > 512; geom_dim > 4; fewer than two hidden layers), < 0 for an invalid net.  The ONE definition of
 * that condition: deep_sdf.utils.decode_sdf (deep_sdf/utils.py:54-65) asks it instead of restating it. */
int dsdf_decode_latent_supported(const DsdfNet* net);

/* ---- module path: Decoder.forward / autograd backward on an explicit input (plugin seam,
 * train_deep_sdf.py:275,514).  forward keeps activations in ws; backward consumes them. */
int dsdf_module_forward(const DsdfNet* net, const float* packed, const float* params, const float* input,
                        int64_t ld_in, int64_t n, int32_t training, const uint32_t* dropout_key /*[host]*/,
                        float* sdf_out, void* ws, size_t ws_bytes, void* stream);
int dsdf_module_backward(const DsdfNet* net, const float* packed, const float* params, const float* d_sdf,
                         int64_t n, int32_t training, const uint32_t* dropout_key /*[host] the forward's keys; only
                         latent_dropout nets read it (slot 15), may be NULL otherwise*/,
                         float* grads /*arena, overwritten or accumulated*/,
                         int32_t accumulate, float* d_input /*[n, ld_din] or NULL*/, int64_t ld_din,
                         void* ws, size_t ws_bytes, void* stream);
/* Forward-mode tangent (Jacobian-vector product) of Decoder.forward at the point of the LAST dsdf_module_forward on this
 * workspace: jvp_out [n] = d sdf / d input . tangent, tangent [n, ld_t] (L+G columns used).  What
 * torch.autograd.functional.jvp computes through the reference decoder in deep_sdf/mesh.py:420 (d vertices / d latent
 * control points) by double backward; here it is one extra pass through the same GEMMs with the primal pass's ReLU /
 * dropout decisions.  May be called any number of times after one forward (before or after dsdf_module_backward). */
int dsdf_module_jvp(const DsdfNet* net, const float* packed, const float* params, const float* tangent, int64_t ld_t,
                    int64_t n, int32_t training, const uint32_t* dropout_key /*[host] as dsdf_module_backward*/,
                    float* jvp_out, void* ws, size_t ws_bytes, void* stream);
/* d_input [n, ld_din] of dsdf_module_backward for an eval-mode dsdf_module_forward (training == 0), with every weight-gradient
 * launch skipped: no gradient arena is read or written.  The dX launches are those of dsdf_module_backward, so d_input is bit for
 * bit what it returns.  One pass of this with d_sdf = 1 gives d sdf / d latent for every row, which replaces the
 * latent_dim x n_control_points double-backward passes of deep_sdf/mesh.py:405-422 (inside :346-454). */
int dsdf_module_input_grad(const DsdfNet* net, const float* packed, const float* params, const float* d_sdf, int64_t n,
                           float* d_input, int64_t ld_din, void* ws, size_t ws_bytes, void* stream);

/* ---- training step ---------------------------------------------------------------------------------
 * dsdf_train_forward_backward = train_deep_sdf.py:509-533 for one chunk: max-norm renorm of the looked-up
 * latent rows (in place), gather + concat, decoder forward, clamp, sum-L1 / n_norm, code regulariser,
 * backward.  grads (decoder arena) and dlat [S_tot, L] are overwritten when accumulate == 0, added to
 * otherwise (--batch_split).  loss_out: device float, same accumulate rule.  sdf_out may be NULL. */
int dsdf_train_forward_backward(const DsdfNet* net, const float* packed, const float* params,
                                float* latent_table, int64_t n_scenes, const DsdfBatch* batch,
                                const DsdfLossCfg* cfg, float* grads, float* dlat, float* loss_out,
                                float* sdf_out, int32_t accumulate, void* ws, size_t ws_bytes, void* stream);

/* clip_grad_norm_ over the decoder arena (train_deep_sdf.py:541-543): writes total norm and the clip
 * coefficient min(1, max_norm/(norm+1e-6)) to two device floats.  ws: one float per block of 4096 gradients, at most 1024
 * of them (4096 bytes always suffice; + one debug red zone when dsdf_debug_ws_redzone is set). */
int dsdf_grad_norm(const float* grads, int64_t n, float max_norm, float* norm_out, float* coef_out,
                   void* ws, size_t ws_bytes, void* stream);

/* optimizer_all.step() (train_deep_sdf.py:545): fused Adam over the decoder arena (lr_decoder) and the
 * WHOLE latent table (lr_latent; dense update, rows absent from the batch keep moving by momentum),
 * then re-materialises the packed weights. */
int dsdf_adam_step(const DsdfNet* net, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                   float* latent_table, const float* dlat, float* lat_exp_avg, float* lat_exp_avg_sq,
                   int64_t n_latent_floats, const DsdfAdamCfg* cfg, float* packed, void* stream);

/* Single-GPU fast path = dsdf_train_forward_backward (accumulate 0) + dsdf_adam_step in one call.  When nothing has to
 * happen between the gradients and the update (no all-reduce, no --batch_split accumulation, no clipping:
 * adam->grad_scale == NULL) the decoder's Adam and the new weight-norm scales are folded into the split-K finalize pass
 * (the gradient arena is then NOT written); otherwise it is exactly the two calls in sequence. */
int dsdf_train_step(const DsdfNet* net, float* packed, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                    float* latent_table, int64_t n_scenes, float* dlat, float* lat_exp_avg, float* lat_exp_avg_sq,
                    const DsdfBatch* batch, const DsdfLossCfg* cfg, const DsdfAdamCfg* adam, float* loss_out, float* sdf_out,
                    void* ws, size_t ws_bytes, void* stream);

/* latent-only Adam (frozen decoder; config 4): updates only the given latent arena. */
int dsdf_adam_latent_only(float* latent, const float* dlat, float* exp_avg, float* exp_avg_sq, int64_t n,
                          const DsdfAdamCfg* cfg, void* stream);

/* The same update for a loop that is CAPTURED INTO A HIP GRAPH and replayed (deepsdf_amd/reconstruct.py: the 800 iterations of a
 * reconstruction are one captured iteration replayed, no host work per iteration): everything that changes from step to step comes
 * from DEVICE memory.  sched [n_steps][2] = { lr_t / (1 - beta1^t), sqrt(1 - beta2^t) } for t = 1 .. n_steps (computed by the caller
 * in double, as dsdf_adam_latent_only does on the host), indexed by the device counter *step_counter (0-based; entries past the end
 * reuse the last one); the call increments the counter after the update (a second, one-thread launch).  The gradient it applies is
 * dlat + l2_coef * latent (the code regulariser l2reg * mean(z^2) of the reconstruction loss; 0: none). */
int dsdf_adam_latent_sched(float* latent, const float* dlat, float* exp_avg, float* exp_avg_sq, int64_t n, const float* sched,
                           int64_t n_steps, int64_t* step_counter, float beta1, float beta2, float eps, float l2_coef, void* stream);

/* ---- diagnostics: per-kernel-class device time from HIP events recorded on the caller's stream around every
 * launch of that class (bench.py's roofline object).  Off by default; thread-local; read synchronises. */
#define DSDF_PROF_CLASSES 8
enum { DSDF_PROF_GEMM_NT = 0, DSDF_PROF_GEMM_TN = 1, DSDF_PROF_LAST = 2, DSDF_PROF_FUSED_FWD = 3, DSDF_PROF_FUSED_BWD = 4,
       DSDF_PROF_DW_STREAM = 5, DSDF_PROF_OTHER = 6, DSDF_PROF_FUSED_FWD_BWD = 7 /* training: forward + backward in one launch */ };
typedef struct DsdfProfile {
  double ms[DSDF_PROF_CLASSES];     /* summed event-to-event time per class */
  double flops[DSDF_PROF_CLASSES];  /* summed ALGORITHMIC 2*M*N*K of the GEMMs each launch covers (the reference's dense form) */
  int64_t count[DSDF_PROF_CLASSES]; /* launches per class */
  int32_t dropped;                  /* 1 if the event pool overflowed (results incomplete) */
} DsdfProfile;
int dsdf_profile_enable(int32_t on);
int dsdf_profile_read(DsdfProfile* out);

/* ---- per-step subsampling --------------------------------------------------------
 * Replaces deep_sdf/data.py:74-110 unpack_sdf_samples + the DataLoader collate (train_deep_sdf.py:483-501) for
 * samples that are resident in HBM: for each of the B scenes, S = 2*(subsample/2) rows -- subsample/2 positives and
 * negatives drawn WITHOUT replacement (the reference's torch.randperm(len)[:n]), a shortfall of one sign made up by
 * the other, positives first -- gathered into xyz_out [B*S, G] / sdf_out [B*S].
 *   data       [rows, G+1] fp32: xyz then sdf; scene k's positives are rows [pos_start[k], pos_start[k]+n_pos[k]),
 *              its negatives [neg_start[k], ...); the four per-scene arrays are int64 on the device
 *   scene_ids  [B] int64 (device): which scenes, in batch order
 *   key        64-bit draw key (e.g. seed and step); the same key gives the same batch
 * The permutation is the keyed Feistel network specified by oracle/deepsdf_oracle.py sample_perm (bit-exact).
 * Every selected scene needs n_pos + n_neg >= S and each sign at most 2^30 rows (checked by the caller, who owns the
 * sizes; the library cannot read device arrays on the host). */
int dsdf_sample_batch(const float* data, int32_t geom_dim, const int64_t* pos_start, const int64_t* n_pos,
                      const int64_t* neg_start, const int64_t* n_neg, const int64_t* scene_ids, int64_t n_batch_scenes,
                      int64_t subsample, uint64_t key, float* xyz_out, float* sdf_out, void* stream);

/* The same draw inside a graph-captured loop (deepsdf_amd/reconstruct.py): the draw key is key0 + *counter * key_step (mod 2^64),
 * *counter a DEVICE integer read by the kernel -- e.g. the step counter dsdf_adam_latent_sched advances -- so every replay of
 * the captured launch draws a new batch, and the sequence equals that of dsdf_sample_batch called with those keys. */
int dsdf_sample_batch_seq(const float* data, int32_t geom_dim, const int64_t* pos_start, const int64_t* n_pos,
                          const int64_t* neg_start, const int64_t* n_neg, const int64_t* scene_ids, int64_t n_batch_scenes,
                          int64_t subsample, uint64_t key0, uint64_t key_step, const int64_t* counter, float* xyz_out, float* sdf_out,
                          void* stream);

/* ---- marching cubes: deep_sdf/mesh.py convert_sdf_samples_to_ply's skimage.measure.marching_cubes, on the device ---------
 * sdf [nx][ny][nz] fp32 (z fastest, axis 0 = x: the reference's reshape(N, N, N)), 2 <= nx, ny, nz <= 1024.  A grid point is
 * inside iff v < level (strictly); one vertex per grid edge whose endpoints lie on different sides, shared by every cell touching
 * it, at origin[a] + (p[a] + t) * spacing[a] along the edge axis a (t = (level - v0) / (v1 - v0), fp32, every operation rounded
 * on its own) and origin[b] + p[b] * spacing[b] on the other two.  Order, without atomics (two runs give identical bytes):
 * vertices by grid-point linear index, then axis x, y, z; faces by cell linear index, then case-table order.  Faces are
 * counter-clockwise seen from increasing sdf (right-hand normals point outward).  Ambiguous cube faces separate the inside corners.
 * Ties, zeros, non-finite values (the rules of dsdf_mc_*, dsdf_tet_*, dsdf_msd_* and dsdf_vd_* alike; tests/grid_values.py):
 *   the fp32 comparison v < level alone decides inside and outside.  A value equal to the level is outside, whichever the sign of
 *   either zero: -0.0f is 0.0f, level = -0.0f is level = 0.0f.  NaN and +inf are outside, -inf is inside.  The faces / elements and
 *   the order and ids of the vertices are functions of that inside pattern alone.
 *   A vertex's coordinates are what the stated sequence gives in IEEE fp32 arithmetic, subnormal numbers included (nothing is
 *   flushed).  A tie gives t = 0 or t = 1 exactly and the vertex sits on the grid point; the sign of a zero t never reaches a
 *   coordinate (p[a] >= +0, and (+0) + (-0) = +0).  A non-finite value changes only the vertices on its own edges: t and the
 *   coordinates along the edge's axes are what the sequence says -- NaN for a NaN value, for an infinite v0 and for -inf against
 *   +inf; t = 0 for a finite v0 against an infinite v1.  Which NaN (sign, payload) is not specified.
 * Use: dsdf_mc_count (writes {n_verts, n_faces} as int64 to device memory), read the totals, allocate, dsdf_mc_emit with the
 * SAME grid, level and workspace (the emit pass reads what the count pass left there).  Totals above INT32_MAX are refused
 * (DSDF_E_INVALID) before anything is written. */
int dsdf_mc_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes);                     /* [host] */
int dsdf_mc_count(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* totals /*[2], device*/, void* ws,
                  size_t ws_bytes, void* stream);
/* verts [n_verts][3] fp32, faces [n_faces][3] int32 (vertex ids); spacing, origin [host] 3 floats each */
int dsdf_mc_emit(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing, const float* origin,
                 int64_t n_verts, int64_t n_faces, float* verts, int32_t* faces, void* ws, size_t ws_bytes, void* stream);
/* The grid edge of every vertex (what deep_sdf/mesh.py:346-454 needs to differentiate the mesh): edge_point [n_verts] int64, the
 * linear index of grid point p, edge_axis [n_verts] int32, the axis a of edge (p, p + e_a), in the vertex order of dsdf_mc_emit.
 * Reads what dsdf_mc_count left in the workspace (the crossing masks and the per-workgroup offsets), so it is valid from
 * dsdf_mc_count to the end of the workspace's life, before or after dsdf_mc_emit; n_verts is the counted total (fewer: the
 * first n_verts).  n_verts == 0 launches nothing. */
int dsdf_mc_edges(int32_t nx, int32_t ny, int32_t nz, int64_t n_verts, int64_t* edge_point, int32_t* edge_axis, void* ws,
                  size_t ws_bytes, void* stream);
/* [host] the compiled-in case table (generated by deepsdf_amd/mc_table.py): *width = entries per case (edge ids of its
 * triangles, -1 terminated); table (may be NULL) receives 256 * width int8. */
int dsdf_mc_case_table(int8_t* table, size_t table_bytes, int32_t* width);

/* ---- mesh SDF: sdf_sampler/sdf_sampler.py SDFfromMesh (igl.point_mesh_squared_distance + an embree inside test), on the device
 * Brute force over every face.  Per query p:
 *   sqr_dist  min over faces of |p - c|^2, c the closest point of the closed triangle, |p - c|^2 from the difference vector;
 *             a zero-area face counts as its longest edge (or its point).  face = the LOWEST index attaining the minimum,
 *             closest = c on that face.
 *   winding   sum over faces of 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|) / 4 pi, a, b, c = vertices - p
 *             (Van Oosterom-Strackee); zero-area faces add nothing, and neither does a face one of whose vertices is p itself
 *             (the angle is undefined there).
 *   sdf       p is inside iff floor(|winding| + 0.5) is odd: sdf = inside ? -sqrt(sqr_dist) : sqrt(sqr_dist), negated when
 *             flip_sign.  For a closed mesh this is the parity of a ray test and does not depend on face orientation.
 * Use: dsdf_msdf_plan, dsdf_msdf_prepare once per mesh (verts [n_verts][3] fp32, faces [n_faces][3] int32, 0-based; indices are
 * clamped into [0, n_verts) on the device -- range-check them on the host), then dsdf_msdf_query as often as needed with the
 * record buffer `tri`.  Every output of dsdf_msdf_query may be NULL, not all of them: sdf needs both passes, winding alone skips
 * the distance work, sqr_dist / face / closest alone skip the winding work.
 * Split rule (n_splits): the query pass runs ceil(n_queries / 256) workgroups of 256 queries; when they are fewer than 2048 the
 * face range is cut into n_splits = min(ceil(2048 / that), floor(n_faces / 1024), 64) contiguous pieces (at least 1), one
 * workgroup per (query block, piece), combined in piece order without atomics: sqr_dist, face and closest do not depend on
 * the split, winding only through its summation order.  Two identical calls give identical bytes.
 * Accuracy and range: a face is zero-area when |ab x ac|^2 <= 1e-14 * (its longest edge)^4, evaluated in fp64 on the fp32
 * vertices.  For every other face -- slivers down to that threshold included -- sqrt(sqr_dist) and closest are good to a few 1e-7
 * of the distance from p to the face's vertices, and winding to ~1e-5 of a turn at distances above 1e-3 of the face's size: the
 * face normal and the denominator of the solid angle are taken in fp64.  The differences p - a are formed first, so a translated
 * mesh costs only the rounding of its fp32 coordinates.  Scaling vertices and queries by a power of two scales sqr_dist, closest
 * and sdf exactly and leaves face and the inside decision unchanged, as long as squared lengths, face areas and their products
 * with a distance (a length cubed) remain normal fp32 numbers: edge lengths and distances within about [2^-30, 2^30].
 * n_faces and n_queries must fit int32.  n_queries == 0 is valid and launches nothing. */
int dsdf_msdf_plan(int64_t n_faces, int64_t n_queries, size_t* tri_bytes, size_t* ws_bytes, int32_t* n_splits); /* [host] */
int dsdf_msdf_prepare(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* tri, size_t tri_bytes,
                      void* stream);
/* queries [n_queries][3]; sdf, sqr_dist, winding [n_queries] fp32; face [n_queries] int32; closest [n_queries][3] fp32 */
int dsdf_msdf_query(const void* tri, int64_t n_faces, const float* queries, int64_t n_queries, float* sdf, float* sqr_dist,
                    int32_t* face, float* closest, float* winding, int32_t flip_sign, void* ws, size_t ws_bytes, void* stream);

/* ---- point sets: the kernels behind deep_sdf/metrics/chamfer.py (scipy KDTree query, trimesh.sample.sample_surface) and the
 * surface half of sdf_sampler.py noisy_sample, on the device (csrc/pointset.hpp) ------------------------------------------------
 * Nearest neighbour, brute force.  For every query q of queries [n_queries][3] against refs [n_refs][3], both fp32:
 *   sqr_dist  min over j of fmaf(dz, dz, fmaf(dy, dy, dx * dx)), (dx, dy, dz) = q - refs[j] formed explicitly (three rounded
 *             subtractions, one rounded product, two fused multiply-adds)
 *   index     the LOWEST j attaining the minimum.  A pair whose value is NaN is never chosen (the test is value < best); a query
 *             with no comparable pair (every value NaN or +inf) reports sqr_dist = +inf, index = 0.
 * sqr_dist [n_queries] fp32, index [n_queries] int32; either may be NULL, not both.
 * Split rule (n_splits): the query pass runs ceil(n_queries / 1024) workgroups of 256 lanes with 4 queries per lane; when they
 * are fewer than 2048 the reference set is cut into n_splits = min(ceil(2048 / that), floor(n_refs / 1024), 64) contiguous pieces
 * (at least 1), one workgroup per (query block, piece), combined in piece order with strict < and without atomics: neither
 * output depends on the split.  Two identical calls give identical bytes.  One piece needs no workspace (ws_bytes = 0, ws may be
 * NULL); more need n_splits * n_queries * 8 bytes.
 * n_queries and n_refs must fit int32.  n_queries == 0 is valid and launches nothing; n_refs == 0 is DSDF_E_INVALID. */
int dsdf_nn_plan(int64_t n_queries, int64_t n_refs, size_t* ws_bytes, int32_t* n_splits);               /* [host] */
int dsdf_nn_query(const float* queries, int64_t n_queries, const float* refs, int64_t n_refs, float* sqr_dist, int32_t* index,
                  void* ws, size_t ws_bytes, void* stream);

/* Mean of n fp32 values as one fp64 on the device (*mean, 8-byte aligned): every value converted to fp64, summed in fp64 by
 * min(ceil(n / 4096), 1024) workgroups over contiguous slices (lane sums in stride order, a fixed tree per workgroup), then the
 * partial sums by one workgroup in the same way, divided by n.  No atomics: two calls give identical bits.  ws is a fixed
 * scratch of DSDF_MEAN_WS_BYTES (8-byte aligned; there is no planner and the debug red zones do not apply).  n == 0 is
 * DSDF_E_INVALID. */
#define DSDF_MEAN_WS_BYTES 8192
int dsdf_mean_f64(const float* x, int64_t n, double* mean, void* ws, size_t ws_bytes, void* stream);

/* Area-weighted sampling of a triangle mesh's surface (verts [n_verts][3] fp32, faces [n_faces][3] int32 as for dsdf_msdf_prepare).
 * dsdf_surf_prepare, once per mesh, fills the `surf` buffer (dsdf_surf_plan: *surf_bytes; 8-byte aligned):
 *   area  [n_faces] fp32 at byte *area_offset: 0.5 * sqrt(n.n), n = ab x ac, ab = b - a, ac = c - a, every product, difference and
 *         sum rounded to fp32 on its own (n.n = (nx nx + ny ny) + nz nz), the square root correctly rounded
 *   cdf   [n_faces] fp64 at byte 0: the inclusive prefix sums of area, formed in fp64 by a fixed three-pass scan over tiles of
 *         1024 faces (*n_tiles = ceil(n_faces / 1024)) -- deterministic, and within n_faces * 2^-53 * total of the exact sums;
 *         total = cdf[n_faces - 1]
 * It waits for the stream, returns the total in *total_area ([host], may be NULL) and fails with DSDF_E_INVALID when the total
 * is 0 or not finite; dsdf_surf_sample is defined only on a buffer it accepted.
 * Sample i = offset + t, t in [0, n), with the 64-bit seed:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (lo32(i), 0, hi32(i), 0), key = (lo32(seed), hi32(seed)))
 *   r = fp64(w0 * 2^32 + w3) * 2^-64 (the integer rounded to nearest), x = r * total rounded to fp64
 *   face = the first f with cdf[f] > x, so a face that adds no area is never chosen; when there is none (r rounded to 1): the
 *          first f with cdf[f] = total, the last face that added area
 *   u = (w1 >> 8) * 2^-24, v = (w2 >> 8) * 2^-24 in fp32; if the fp32 sum u + v > 1: u = 1 - u, v = 1 - v
 *   p = fmaf(ac, v, fmaf(ab, u, a)) per coordinate, the nesting of the mesh SDF's closest point
 * std > 0 adds std * N(0, 1) per coordinate (fmaf(std, g, p)): (g0, g1, g2, g3) = Philox4x32-10 with counter (lo32(i), 1, hi32(i),
 * 0), Box-Muller in fp32: x = sqrt(-2 log(((g0 >> 8) + 1) 2^-24)) cos(2 pi (g1 >> 8) 2^-24), y = the same radius times the sine,
 * z = sqrt(-2 log(((g2 >> 8) + 1) 2^-24)) cos(2 pi (g3 >> 8) 2^-24).  std == 0 draws nothing and changes no bit.
 * Sample i depends on (seed, i, mesh) only: n samples at offset 0 and n at offset n equal 2 n samples at offset 0.
 * points [n][3] fp32; face [n] int32 and bary [n][2] fp32 (u, v) may be NULL.  n must fit int32; n == 0 launches nothing. */
int dsdf_surf_plan(int64_t n_faces, size_t* surf_bytes, size_t* area_offset, int32_t* n_tiles);          /* [host] */
int dsdf_surf_prepare(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, void* surf, size_t surf_bytes,
                      double* total_area, void* stream);
int dsdf_surf_sample(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const void* surf, size_t surf_bytes,
                     int64_t n, uint64_t offset, uint64_t seed, float std_dev, float* points, int32_t* face, float* bary,
                     void* stream);

/* ---- microstructure grids: deep_sdf/mesh.py create_mesh_microstructure / analysis/geometry.py sdf_struct, the parts in front of
 * and behind the decoder (csrc/msgrid.hpp) ----------------------------------------------------------------------------------
 * The padded grid has dims[a] = N[a] + 2 points per axis (linear index, z fastest).  Unfolded coordinate of index i on axis a:
 *   xo = (fp32(i) * voxel_size) + voxel_origin, voxel_size = 2 / (dims[a] - 3), voxel_origin = -1 - voxel_size, both computed in
 *   double and rounded to fp32 once; one rounded multiply and one rounded add, never an FMA.
 * Folded coordinate, t = tiling[a], p = 2 / t:  (2/p) * |((xo - t%2) mod 2p) - p| - 1, mod the floored remainder (fmodf, plus 2p
 * when the result is non-zero and negative), every operation rounded on its own, constants rounded from double once.
 * Inside: -1 <= xo <= 1 on all three axes.
 * dsdf_ms_rows writes rows [n][L + 3] (or [n][L] when with_xyz == 0) fp32 = [spline(xo) | folded xo]:
 *   grid mode   (points == NULL): points [start, end) of the padded grid, n = end - start; rows of outside points have exact
 *               zeros in the latent columns (inside_test is ignored: it is always on)
 *   point mode  (points != NULL, device [n][3], n = end - start, start is ignored): xo is the given point.  inside_test != 0: as
 *               the grid; inside_test == 0: every row gets the spline at the point clamped to the knot range (sdf_struct).
 * The spline: degree 1..3 per axis, knot vectors with n_cp[a] + degree[a] + 1 non-decreasing entries and a non-empty range
 * knots[degree] < knots[n_cp]; control points cp [ncp][L], ncp = n_cp[0] * n_cp[1] * n_cp[2], first parametric axis fastest.
 * The parametric coordinate is clamped to the knot range and the span search stops at the last non-empty span, so the right
 * end evaluates to the end value.  knots_host are checked on the host; knots_dev is the device copy the kernel reads (the three
 * vectors one after another, axis 0 first) and must hold the same values.
 * dsdf_ms_caps works in place on sdf [end - start], the values of grid points [start, end): first the n_caps records in the
 * order given -- border = (xo[dim] - c) * -m; cap -1: sdf = max(sdf, -border); cap 1: sdf = min(sdf, border); m = -1 or 1,
 * c = m * (1 - measure) rounded from double by the caller -- then the six planes of the unit cube with max (x-, x+, y-, y+,
 * z-, z+).  Every argument error returns DSDF_E_INVALID before anything is launched. */
#define DSDF_MS_MAX_CAPS 6
typedef struct DsdfMsGrid {
  int32_t dims[3];                 /* padded: N + 2, each 4 .. 1024 */
  int32_t tiling[3];               /* >= 1 */
} DsdfMsGrid;

typedef struct DsdfMsSpline {
  int32_t degree[3];               /* 1 .. 3 */
  int32_t n_cp[3];                 /* control points per axis, > degree */
  int32_t n_knots[3];              /* must equal n_cp + degree + 1 */
  const float* knots_host[3];      /* [host] */
  const float* knots_dev;          /* device, n_knots[0] + n_knots[1] + n_knots[2] floats */
  const float* cp;                 /* device [ncp][L] */
  int64_t ncp;                     /* must equal n_cp[0] * n_cp[1] * n_cp[2] */
  int32_t L;                       /* >= 1 */
} DsdfMsSpline;

typedef struct DsdfMsCap {
  int32_t dim;                     /* 0 .. 2 */
  int32_t cap;                     /* -1 or 1 */
  float m;                         /* -1 or 1 */
  float c;                         /* m * (1 - measure) */
} DsdfMsCap;

int dsdf_ms_rows(const DsdfMsSpline* spline, const DsdfMsGrid* grid, int64_t start, int64_t end, const float* points,
                 int32_t inside_test, int32_t with_xyz, float* rows, void* stream);
int dsdf_ms_caps(const DsdfMsGrid* grid, int64_t start, int64_t end, const DsdfMsCap* caps /*[host]*/, int32_t n_caps, float* sdf,
                 void* stream);

/* Grid mode for a list of padded-grid linear indices (device int64 [n], any order, repeats allowed): rows [n][L + 3] are bit
 * for bit those of dsdf_ms_rows' grid mode at these indices (the unfolded coordinate comes from the index with the single-rounded
 * arithmetic above, never from a point list).  Also written, when not NULL: weights [n][64] fp32, the tensor-product basis weight
 * of control point (first + (i, j, k)) in slot (k * 4 + j) * 4 + i, zero in unused slots, and base [n] int32, the linear index of
 * the first control point (first parametric axis fastest), -1 for outside points (weights all zero).  An index outside the grid
 * cannot be refused on the host: its row and weights are zero and its base is -1.  n == 0 launches nothing.
 * Replaces the spline evaluation of deep_sdf/mesh.py:346-454 (create_mesh_microstructure_diff) on the band of grid points. */
int dsdf_ms_rows_at(const DsdfMsSpline* spline, const DsdfMsGrid* grid, const int64_t* indices, int64_t n, float* rows,
                    float* weights, int32_t* base, void* stream);

/* ---- derivative of a microstructure mesh with respect to the spline's control points (csrc/msdiff.hpp) ---------------------
 * deep_sdf/mesh.py:346-454 (create_mesh_microstructure_diff: latent_dim x n_control_points double-backward passes over the grid,
 * :405-422), assembled in closed form.  Vertex v lies on edge (p, a) = (edge_point[v], edge_axis[v]) of the capped grid, between
 * s0 = grid[p] and s1 = grid[p + e_a]; only coordinate a moves:
 *   J[v, c, l] = scale[a] * sum_{k in {0, 1}} dt/ds_k * mask_k * G_k[l] * weight_k(c)
 *   dt/ds0 = (level - s1) / (s1 - s0)^2,  dt/ds1 = -(level - s0) / (s1 - s0)^2  (fp32, from the two values marching cubes read)
 * where k names the band row band_of[p] / band_of[p + e_a].  Band row r carries G [r][0 .. L) = d sdf / d latent at the row the
 * forward decoded, the weights and base of dsdf_ms_rows_at, and mask (1: inside and the caps left the decoder's value).
 * A vertex whose edge, band row or base is out of range gets zeros; nothing is read out of bounds for in-range arrays.  In range:
 * an edge with 0 <= a <= 2, 0 <= p < npts and p's index along axis a below dims[a] - 1 (the rule of dsdf_vd_* below: an edge at
 * the last index of an axis is refused on every axis, also where p + e_a would be the first point of the next row); an endpoint
 * whose band_of row lies in 0 .. n_band - 1, with mask != 0, 0 <= base < ncp and base's index + degree < n_cp on every axis.  A
 * vertex out of range reports axis a when 0 <= a <= 2 and axis 0 otherwise.
 * Ties: the comparison rules are dsdf_mc_*'s ("Ties, zeros, non-finite values", above); an endpoint whose value equals the level
 * (either zero) gives the OTHER endpoint the factor dt/ds = 0 exactly.  Not part of the contract: what a difference s1 - s0 outside
 * fp32's normal range gives.  Today the dt pair is formed as d = s1 - s0, d * d, the numerator, the quotient, so a subnormal d gives
 * +-inf or NaN and an overflowed d gives 0 (observed, tests/test_gpu_grid_values.py); only that such a vertex leaves every other
 * vertex's results untouched is promised.
 *   dsdf_msd_jacobian  jac [n_verts][ncp][L] and axis [n_verts] (may be NULL); full != 0: jac [n_verts][3][ncp][L], the two other
 *                      coordinates' planes written as zeros (the reference's layout)
 *   dsdf_msd_jvp       d_cp [ncp][L] -> d_verts [n_verts][3] (zeros off the edge axis)
 *   dsdf_msd_vjp       grad_verts [n_verts][3] -> grad_cp [ncp][L]; two stages: ceil(n_verts / 512) partial sums in vertex order, then
 *                      their sum in part order; ws from dsdf_msd_vjp_workspace_bytes (256-byte aligned, planner conventions:
 *                      dsdf_debug_ws_redzone / dsdf_debug_ws_regions)
 * No atomics; two identical calls give identical bytes.  Every argument error returns DSDF_E_INVALID before anything is launched. */
typedef struct DsdfMsdMesh {
  const float* grid;               /* device, capped sdf [dims[0]][dims[1]][dims[2]] */
  const int64_t* edge_point;       /* device [n_verts] */
  const int32_t* edge_axis;        /* device [n_verts] */
  const int32_t* band_of;          /* device [grid points]: band row of a grid index, < 0: none */
  int64_t n_verts;
  int32_t dims[3];                 /* 2 .. 1024 */
  float scale[3];                  /* voxel_size / 2 of the returned vertices */
  float level;
} DsdfMsdMesh;

typedef struct DsdfMsdBand {
  const float* G;                  /* device [n_band][ld_g] */
  const float* weights;            /* device [n_band][64] */
  const int32_t* base;             /* device [n_band] */
  const uint8_t* mask;             /* device [n_band] */
  int64_t n_band, ld_g;
  int32_t degree[3], n_cp[3];
  int32_t L;
} DsdfMsdBand;

int dsdf_msd_vjp_workspace_bytes(int64_t n_verts, int64_t n_control_points, int32_t L, size_t* bytes, int32_t* n_parts); /* [host] */
int dsdf_msd_jacobian(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, int32_t full, float* jac, int32_t* axis, void* stream);
int dsdf_msd_jvp(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, const float* d_cp, float* d_verts, void* stream);
int dsdf_msd_vjp(const DsdfMsdMesh* mesh, const DsdfMsdBand* band, const float* grad_verts, float* grad_cp, void* ws,
                 size_t ws_bytes, void* stream);

/* ---- surface topology and geometry: the surface half of analysis/geometry.py DeepSDFMesh (trimesh's face_adjacency, connected
 * components, is_watertight, vertex_normals; the volume and the normal-projected shape derivative), on the device (csrc/meshtopo.hpp)
 * verts [n_verts][3] fp32, faces [n_faces][3] int32 as for dsdf_msdf_prepare; n_faces <= INT32_MAX / 3.  Every index read from a
 * caller's array (face indices, order, corner_order, vstart, mate, axis) is clamped into its range on the device before it is used
 * as an address: a badly sorted or out-of-range array gives an unspecified result and no access outside the arrays.  Sorting is
 * the caller's (a stable sort); the entries take the sorted arrays.  n_faces == 0 launches nothing.  No floating-point atomics
 * anywhere; two identical calls give identical bytes.
 *   dsdf_mt_plan             [host] one workspace (256-byte aligned, planner conventions: dsdf_debug_ws_redzone / _regions) serves
 *                            dsdf_mt_adjacency, dsdf_mt_components and dsdf_mt_volume of a mesh of n_faces faces
 *   dsdf_mt_edge_keys        keys [3 n_faces] int64: half-edge h = 3 f + k runs faces[f][k] -> faces[f][(k + 1) % 3]; its key is
 *                            (min << 32) | max of the two vertex ids, -1 when they are equal (an index-degenerate face)
 *   dsdf_mt_adjacency        sorted_keys [3 n_faces] = the keys in non-decreasing order, order [3 n_faces] int64 = the half-edge at each
 *                            sorted position.  mate [3 n_faces] int32: a half-edge whose key is >= 0 and occurs exactly twice gets the
 *                            other half-edge of that key, every other one -1 (trimesh's face_adjacency: an edge of one face or of more
 *                            than two joins nothing).  stats [6] int64 (device): distinct edges, boundary edges (one face), non-manifold
 *                            edges (more than two), paired edges, paired edges whose two half-edges run in the SAME direction
 *                            (inconsistent winding), half-edges with key -1.  Watertight: the boundary, non-manifold and key -1
 *                            counts are 0; winding-consistent: also the same-direction count.  Integer sums in a fixed order.
 *   dsdf_mt_components       label [n_faces] int32: the lowest face index of the face's component under the mate relation; size
 *                            [n_faces] int32 (may be NULL): the face count of the component whose lowest face is r at r, 0 elsewhere.
 *                            Min-hooking with shortcutting, repeated until a round changes nothing; *n_rounds ([host], may be NULL) =
 *                            the rounds run, the unchanged one included.  int32 atomicMin / atomicAdd decide only the order of the
 *                            work: the fixed point and the sizes do not depend on it.  This entry WAITS FOR THE STREAM: it reads the
 *                            rounds' change flags on the host, four rounds at a time (as dsdf_surf_prepare reads its total).
 *   dsdf_mt_face_degenerate  out [n_faces] uint8: 1 for a face with a repeated index or of zero area by the mesh SDF's rule,
 *                            |ab x ac|^2 <= 1e-14 (longest edge)^4 in fp64 on the fp32 vertices; 0 otherwise
 *   dsdf_mt_vertex_geometry  corner_order [3 n_faces] int64: the corners 3 f + k stably sorted by their vertex, vstart [n_verts + 1]
 *                            int64: the start of every vertex's run.  Per vertex, over its corners in that order, in fp64: corner a of
 *                            face (a, b, c) in cyclic order, e1 = b - a, e2 = c - a, n = e1 x e2:
 *                              normals  [n_verts][3] (may be NULL): s = sum atan2(|n|, e1 . e2) n / |n| over the faces that are not
 *                                       zero-area, s / |s| rounded to fp32 once; exactly 0 when s = 0 or the vertex has no corner
 *                              vol_grad [n_verts][3] (may be NULL): d volume / d vertex = (1 / 6) sum b x c over every corner
 *                                       (absolute positions, zero-area faces included), rounded to fp32 once
 *   dsdf_mt_volume           *volume (device double, 8-byte aligned) = (1 / 6) sum_f a . (b x c) in fp64: min(ceil(n_faces / 4096),
 *                            1024) workgroup sums over contiguous slices, then their sum by one workgroup (dsdf_mean_f64's shape)
 *   dsdf_mt_project          jac [n_verts][R], axis [n_verts]: dsdf_msd_jacobian's (full = 0), R = ncp * L.  With a = axis[v]:
 *                            j = jac[v][r] * stretch[a]; if clip > 0 and |j| > clip: j = 0 (the reference's outlier rule, after the
 *                            stretch); out [n_verts][3][R]: out[v][d][r] = (j * n[a]) * n[d], every product rounded to fp32 on
 *                            its own.  stretch [host] 3 floats.  n_verts == 0 launches nothing.
 * Every argument error returns DSDF_E_INVALID before anything is launched. */
int dsdf_mt_plan(int64_t n_verts, int64_t n_faces, size_t* ws_bytes);                                  /* [host] */
int dsdf_mt_edge_keys(const int32_t* faces, int64_t n_faces, int64_t n_verts, int64_t* keys, void* stream);
int dsdf_mt_adjacency(const int32_t* faces, int64_t n_faces, const int64_t* sorted_keys, const int64_t* order, int32_t* mate,
                      int64_t* stats, void* ws, size_t ws_bytes, void* stream);
int dsdf_mt_components(const int32_t* mate, int64_t n_faces, int32_t* label, int32_t* size, int32_t* n_rounds /*[host]*/, void* ws,
                       size_t ws_bytes, void* stream);
int dsdf_mt_face_degenerate(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, uint8_t* out, void* stream);
int dsdf_mt_vertex_geometry(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const int64_t* corner_order,
                            const int64_t* vstart, float* normals, float* vol_grad, void* stream);
int dsdf_mt_volume(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, double* volume, void* ws,
                   size_t ws_bytes, void* stream);
int dsdf_mt_project(const float* jac, const int32_t* axis, const float* normals, int64_t n_verts, int64_t R,
                    const float* stretch /*[host]*/, float clip, float* out, void* stream);

/* ---- surface following on blocks of the dense grid (csrc/sparsegrid.hpp): the reference builds the coordinates of ALL N^3 grid
 * points and decodes every one of them (deep_sdf/mesh.py:42-70 for create_mesh, :262-271 for the microstructure grid); these
 * entries find the points a mesh needs, so that only those are decoded.  Nothing here evaluates an SDF: the caller decodes the
 * listed points with the entries above and hands the values back.  Additions only: DSDF_ABI_VERSION is unchanged.
 *
 * Grid [nx][ny][nz] fp32, z fastest, 2 .. 1024 points per axis; block edge `block` >= 2 cells.  Coarse coordinates of axis a:
 * {0, block, 2 block, ... < n_a - 1} + {n_a - 1}; block (I, J, K), linear (I * nb_y + J) * nb_z + K, owns the closed point box between
 * consecutive coarse coordinates (the last block of an axis may be short; neighbours share their face points).  Inside: v < level.
 * One workspace (dsdf_sg_plan, 256-byte aligned, planner conventions: dsdf_debug_ws_redzone / _regions) carries the state of one
 * surface-following run between the calls: a state byte per block (0 inactive, 1 new, 2 valued) and a byte per grid point
 * (1: the point holds a decoded value).  The order of a run:
 *   dsdf_sg_plan          [host] block counts, coarse-lattice size, workspace bytes, and where in it the states and the point map lie
 *   dsdf_sg_coarse        indices [n_coarse] int64: the coarse lattice's linear indices, ascending; clears the point map and marks them
 *   (decode, dsdf_sg_scatter)
 *   dsdf_sg_seed          state = 1 for a block whose 8 corners are not all inside or all outside, or whose
 *                         min over corners of fabsf(v - level) <= thr (fp32); 0 otherwise.  *n_new (device int64): blocks in state 1
 *   per round, while *n_new > 0 (the caller reads the two counts on the host: one stream wait per round):
 *     dsdf_sg_points_count  *n_points (device int64): grid points without a value inside blocks of state 1
 *     dsdf_sg_points_emit   indices [n] int64, n = that count: those points, ascending; marks them.  Nothing is written past n.
 *     (decode, dsdf_sg_scatter)
 *     dsdf_sg_grow          gather form: an inactive block becomes 1 if a face-neighbour in state 1 has mixed inside flags among
 *                           the points of the shared face; the blocks that were 1 become 2.  *n_new: blocks newly in state 1
 *   dsdf_sg_fill          every point without a value takes the value at the low corner of the lowest-index block that contains it
 * and, independent of a run:
 *   dsdf_sg_coords        xyz [n][3] of listed points: fp32 index * voxel_size[a], then + origin[a], each rounded on its own
 *                         (voxel_size, origin: [host] 3 floats); nx .. nz >= 1
 *   dsdf_sg_scatter       sdf[indices[q]] = values[q]; an index outside [0, n_points) writes nothing.  Indices must be distinct.
 *   dsdf_sg_caps_at       dsdf_ms_caps' arithmetic, bit for bit, in place on sdf [n], the values of the listed points of the padded grid
 * One thread per block or per point, integer work and plain stores; no atomics: counts are per-workgroup totals summed in a
 * fixed order, so two identical runs give identical bytes.  Every argument error returns DSDF_E_INVALID before anything is launched. */
typedef struct DsdfSgPlan {
  int32_t blocks[3];
  int64_t n_blocks, n_coarse, n_points;
  size_t ws_bytes;
  size_t state_offset, have_offset; /* where the workspace holds the block states [n_blocks] and the point map [n_points], one byte each */
} DsdfSgPlan;

int dsdf_sg_plan(int32_t nx, int32_t ny, int32_t nz, int32_t block, DsdfSgPlan* plan);                  /* [host] */
int dsdf_sg_coarse(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t* indices, void* ws, size_t ws_bytes, void* stream);
int dsdf_sg_seed(const float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, float level, float thr, int64_t* n_new, void* ws,
                 size_t ws_bytes, void* stream);
int dsdf_sg_grow(const float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, float level, int64_t* n_new, void* ws,
                 size_t ws_bytes, void* stream);
int dsdf_sg_points_count(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t* n_points, void* ws, size_t ws_bytes, void* stream);
int dsdf_sg_points_emit(int32_t nx, int32_t ny, int32_t nz, int32_t block, int64_t n, int64_t* indices, void* ws, size_t ws_bytes,
                        void* stream);
int dsdf_sg_fill(float* sdf, int32_t nx, int32_t ny, int32_t nz, int32_t block, void* ws, size_t ws_bytes, void* stream);
int dsdf_sg_coords(int32_t nx, int32_t ny, int32_t nz, const float* voxel_size /*[host]*/, const float* origin /*[host]*/,
                   const int64_t* indices, int64_t n, float* xyz, void* stream);
int dsdf_sg_scatter(const int64_t* indices, int64_t n, const float* values, float* sdf, int64_t n_points, void* stream);
int dsdf_sg_caps_at(const DsdfMsGrid* grid, const int64_t* indices, int64_t n, const DsdfMsCap* caps, int32_t n_caps, float* sdf,
                    void* stream);

/* ---- tetrahedral volume mesh of the solid {sdf < level} (csrc/tetmesh.hpp; numpy restatement: tests/tet_numpy.py) ------------
 * The grid, level, spacing and origin are dsdf_mc_*'s: sdf [nx][ny][nz] fp32, z fastest, 2 <= n <= 1024 per axis, a grid point
 * is inside iff v < level (strictly); spacing > 0.  Additions only: DSDF_ABI_VERSION is unchanged.
 *
 * Kuhn tetrahedra.  Every cell is cut into six tetrahedra around its diagonal (0,0,0)-(1,1,1): for the permutation pi of the axes
 *   (the six of them in lexicographic order) the corners are q0 = cell origin, q1 = q0 + e_pi0, q2 = q1 + e_pi1, q3 = q2 + e_pi2,
 *   and det(q1 - q0, q2 - q0, q3 - q0) = sign(pi): the orientation of everything emitted follows from the permutation's parity
 *   and from integer relabellings, never from a floating-point test.  The triangulation is translation invariant and conforming
 *   across cells.
 * Edges.  A tetrahedron edge is (p, c): its lower grid point p and a class c in 1..7 with direction d = (c & 1, (c >> 1) & 1,
 *   (c >> 2) & 1) -- three axis classes (1, 2, 4), three face diagonals, one body diagonal.  It crosses iff exactly one end is inside.
 * Vertices, in output order: for every grid point in linear order the grid point itself if it is inside (class 0), at
 *   origin + idx * spacing, then its crossing edges in increasing c, at t = (level - v_p) / (v_q - v_p): coordinate b is
 *   origin[b] + (idx[b] + t) * spacing[b] where d[b] = 1 and origin[b] + idx[b] * spacing[b] elsewhere, fp32, every operation
 *   rounded on its own, in dsdf_mc_emit's sequence: the class-1/2/4 vertices are, in order and bit for bit, dsdf_mc_emit's vertices.
 *   t_clamp = tau in [0, 0.5): when tau > 0, t is clamped to [tau, 1 - tau] (1 - tau in fp32) before it is used; tau = 0 does not
 *   touch t.  The clamp bounds how thin a cut element can get and moves the surface by at most tau of an edge.  It is
 *   compare-and-select: t = t < tau ? tau : t, then t = t > hi ? hi : t with hi = 1 - tau.  A NaN t fails both comparisons and
 *   stays NaN under every t_clamp ("a NaN sdf stays", as dsdf_ms_caps has it); fminf / fmaxf would turn it into tau.
 * Elements of a Kuhn tetrahedron by its inside corners (corner numbers in increasing order within "inside" and within "outside";
 *   XY is the vertex on edge XY): none: nothing; all four: (q0, q1, q2, q3); one, A: (A, AB, AC, AD); three, D outside: the prism
 *   (A, B, C | AD, BD, CD); two, A and B: the prism (A, AC, AD | B, BC, BD).  A prism (a0, a1, a2 | b0, b1, b2) with vertical edges
 *   ai-bi is relabelled -- the triangles exchanged if the lowest of its six output ids is a b, then both rotated -- so that a0 is that
 *   lowest id; it gives (a0, b0, b1, b2) and then, if the lowest id of the quadrilateral (a1, a2, b2, b1) is a1 or b2, (a0, a1, a2, b2)
 *   and (a0, a1, b2, b1), else (a0, a1, a2, b1) and (a0, a2, b2, b1): on every quadrilateral the diagonal leaves from the lowest id,
 *   and ids are a global total order, so neighbours agree.  Every element is stored positively oriented (its last two ids exchanged
 *   where the parity says it is negative).  At most 3 elements per Kuhn tetrahedron, 18 per cell.
 * Boundary triangles, outward: the cut faces -- one inside corner (AB, AC, AD), three (AD, BD, CD), two the quadrilateral
 *   (AC, AD, BD, BC), rotated to its lowest id and cut from there -- which face increasing sdf as dsdf_mc_emit's do, kind 0; and
 *   the inside part of every Kuhn face lying in one of the six outer planes of the grid (walk round the outward-ordered face, keep
 *   inside corners and crossing vertices; a quadrilateral is cut as above), kind 1..6 = -x, +x, -y, +y, -z, +z.
 * Order, without atomics (two runs give identical bytes): elements by cell (linear index of its lower corner), permutation, then
 *   the order above; boundary triangles by cell, permutation, cut faces, then the low-plane face (q0, q1, q2), then the high-plane
 *   face (q1, q2, q3).
 * Degenerate input: a value equal to level is outside (of either sign of zero; level = -0.0f is level = 0.0f), so t can be exactly
 *   0 or 1; the vertex then sits on the grid point, the elements touching that point have zero volume and are still emitted (the
 *   topology stays conforming).  With tau > 0 there are none.  Non-finite values: dsdf_mc_*'s rules above -- NaN and +inf are
 *   outside, -inf is inside; tets, bfaces, bface_kind, vert_point, vert_class and the vertex ids are functions of the inside
 *   pattern alone, and a non-finite value changes nothing in verts but the vertices on its own edges.  dsdf_tet_components uses
 *   the same comparison.
 * Use: dsdf_tet_count (writes {n_verts, n_tets, n_bfaces} as int64 to device memory), read the totals, allocate, dsdf_tet_emit with
 * the SAME grid, level and workspace.  Totals above INT32_MAX and a t_clamp outside [0, 0.5) are refused (DSDF_E_INVALID) before
 * anything is launched; nothing is written past n_verts / n_tets / n_bfaces entries.  The workspace (about 11 bytes per grid point,
 * regions tet_* of dsdf_debug_ws_regions) also serves dsdf_tet_components, which overwrites none of what dsdf_tet_count left. */
int dsdf_tet_workspace_bytes(int32_t nx, int32_t ny, int32_t nz, size_t* bytes);                    /* [host] */
int dsdf_tet_count(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int64_t* totals /*[3], device*/, void* ws,
                   size_t ws_bytes, void* stream);
/* verts [n_verts][3] fp32, tets [n_tets][4] int32, bfaces [n_bfaces][3] int32, bface_kind [n_bfaces] int8; vert_point [n_verts]
 * int64 / vert_class [n_verts] int32 (each may be NULL): the grid point p and the class c (0: a grid vertex) of every vertex id;
 * spacing, origin [host] 3 floats each.  tets must be 16-byte aligned (an element is stored as one 16-byte vector; a misaligned
 * pointer is refused with DSDF_E_INVALID); the other arrays need their element's alignment only.
 * n_verts / n_tets / n_bfaces are the counted totals, or fewer to receive only the first entries.  The INT32_MAX check is made on
 * these arguments: the library cannot read the device totals on the host.  A caller who passes FEWER than the counted totals must
 * have checked that the counted totals themselves fit int32 -- beyond that the ids wrap and the entries written are meaningless
 * (still none outside the buffers).  deepsdf_amd.tetmesh.tetrahedralize always passes the counted totals. */
int dsdf_tet_emit(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, const float* spacing, const float* origin,
                  float t_clamp, int64_t n_verts, int64_t n_tets, int64_t n_bfaces, float* verts, int32_t* tets, int32_t* bfaces,
                  int8_t* bface_kind, int64_t* vert_point, int32_t* vert_class, void* ws, size_t ws_bytes, void* stream);
/* Connected components of the solid: two inside grid points joined by a Kuhn edge (p, p + d(c)) are connected (14 neighbours; two
 * inside corners of a Kuhn tetrahedron are always joined by one, and every element holds an inside corner, so these are exactly the
 * components of the mesh).  dsdf_mt_components' conventions: label [npts] int32, the lowest linear index of the point's component,
 * -1 outside; size [npts] int32 (may be NULL), the component's inside-point count at its root, 0 elsewhere; *n_rounds [host] the
 * hooking rounds run.  The result is unique; waits for the stream. */
int dsdf_tet_components(const float* sdf, int32_t nx, int32_t ny, int32_t nz, float level, int32_t* label, int32_t* size,
                        int32_t* n_rounds /*[host]*/, void* ws, size_t ws_bytes, void* stream);

/* ---- P1 linear elasticity on a tetrahedral mesh (csrc/fem.hpp; numpy / scipy restatement: tests/fem_numpy.py) ------
 * Replaces, for order-1 tetrahedra and constant Lame coefficients, what the reference does through mfem in
 * analysis/MFEMLinearElasticity.py.  fp64 throughout; no floating-point atomics; every sum over the mesh runs in a fixed order, so
 * two identical calls give identical bytes.  Additions only: DSDF_ABI_VERSION is unchanged.
 *
 * Mesh: verts [n_verts][3] fp64, tets [n_tets][4] int32 (16-byte aligned), bfaces [n_bfaces][3] int32 (outward); counts fit int32.
 *   corner_order [4 n_tets] int64: the corners c = 4 e + a stably sorted by their vertex tets[e][a]; vstart [n_verts + 1] int64: the
 *   first sorted corner of every vertex (dsdf_mt_vertex_geometry's pair, on the elements); bcorner_order [3 n_bfaces] / bvstart
 *   the same for the boundary triangles.  Every index read from memory is clamped into its range before it is used as an address.
 * Element: e_k = x_k - x_0, c1 = e2 x e3, c2 = e3 x e1, c3 = e1 x e2, det = (e1.x c1.x + e1.y c1.y) + e1.z c1.z, V = det / 6,
 *   g_k = c_k / det (k = 1..3), every operation rounded on its own; g_0 = -((g_1 + g_2) + g_3).  geom [10][n_tets] holds g_1, g_2,
 *   g_3 and V.  An element with V <= 0 or a non-finite gradient is skipped: stored as zeros, counted, and absent from everything below.
 *   K_ab[i][j] = V (lam g_a,i g_b,j + mu g_b,i g_a,j + mu (g_a . g_b) delta_ij).
 * Operator: A = P K P + (I - P); P zeroes the three components of every masked vertex: the fixed ones and the held ones (a vertex
 *   left with no element that counts).  y = A x as V sigma(P x) per element (sigma = lam tr(H) I + mu (H + H^T), H = sum_b x_b g_b^T),
 *   then per vertex the sum of (V sigma)_e g_a over its corners in corner_order's order.
 * Preconditioner: per vertex D = sum of K_aa over its corners, six values (xx, yy, zz, xy, xz, yz), and its inverse; masked vertices
 *   carry the identity in both. */
typedef struct {
  const int32_t* tets;          /* [n_tets][4] */
  const int64_t* corner_order;  /* [4 n_tets] */
  const int64_t* vstart;        /* [n_verts + 1] */
  const double* geom;           /* [10][n_tets]   dsdf_fem_setup's */
  const double* dinv;           /* [n_verts][6]   dsdf_fem_setup's */
  const uint8_t* mask;          /* [n_verts]      dsdf_fem_setup's */
  int64_t n_verts, n_tets;
  double lam, mu;
} DsdfFemOp;
/* One workspace (256-byte aligned; planner conventions, regions fem_*) serves every dsdf_fem_* call on a mesh of these sizes.
 * Replaces nothing in the reference: mfem allocates as it goes. */
int dsdf_fem_plan(int64_t n_verts, int64_t n_tets, int64_t n_bfaces, size_t* ws_bytes);                 /* [host] */
/* Element geometry, preconditioner and mask of `op` (its geom, dinv and mask are WRITTEN here: pass the buffers; lam, mu finite,
 * mu > 0, lam + 2 mu > 0); fixed [n_verts] uint8 or NULL; diag [n_verts][6]; counts [2] int64 on the device: skipped
 * elements, held vertices.  Replaces ElasticityIntegrator's assembly and FormLinearSystem's elimination of the essential dofs
 * (MFEMLinearElasticity.py:308-315) and the smoother's set-up (:318). */
int dsdf_fem_setup(const DsdfFemOp* op, const double* verts, const uint8_t* fixed, double* diag, int64_t* counts, void* ws,
                   size_t ws_bytes, void* stream);
/* y = A x, x and y [n_verts][3], x != y.  The operator the CG of MFEMLinearElasticity.py:319-326 multiplies by. */
int dsdf_fem_apply(const DsdfFemOp* op, const double* x, double* y, void* ws, size_t ws_bytes, void* stream);
/* f [n_verts][3] = sum over the vertex's boundary triangles with face_sel[f] != 0 (NULL: all) of area_f / 3 * traction ([host] 3
 * doubles), 0 at vertices with mask[v] != 0 (NULL: none): VectorBoundaryLFIntegrator with a constant coefficient on the marked
 * attributes (MFEMLinearElasticity.py:304-306), on P1. */
int dsdf_fem_load(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                  const int64_t* bvstart, const uint8_t* face_sel, const double* traction, const uint8_t* mask, double* f, void* stream);
/* Preconditioned CG for A u = P f from u = 0 with MFEM's CGSolver rule (MFEMLinearElasticity.py:319-326: rel_tol 1e-10, 10000
 * iterations): stop when <z, r> <= rel_tol^2 <z0, r0>.  rho, alpha, beta, the iteration count and a done flag live on the device; the
 * kernel that updates them sets done on convergence, on p . A p <= 0 and on a <z, r> that is negative or not a number, and every
 * later kernel returns at once, so u and the count do not depend on check_every (>= 1: the host reads the flag every check_every
 * iterations).  *iterations, *converged, *ratio = <z, r> / <z0, r0> are [host]; waits for the stream.
 * What comes back (tests/test_gpu_fem_cg.py): f = 0 at every unmasked vertex: (0, 1, 0.0), u = 0.  <z0, r0> not a
 * positive number (a NaN in f at an unmasked vertex): (0, 0, 0.0), u = 0.  p . A p <= 0 after j iterations: (j, 0, ratio of iteration
 * j), u iterate j.  max_iter reached: (max_iter, 0, ratio), u that iterate; max_iter = 0: (0, 0, 1.0), u = 0.  A finite f so large
 * that <z0, r0> and p . A p overflow to +inf: alpha is inf / inf, the solve ends after ONE iteration with (1, 0, NaN) and u is NaN at
 * every vertex, the masked ones included -- check *converged before using u.  f at a masked vertex is dropped by selection, not by a product:
 * a value there that is not finite changes nothing.  Every call starts from nothing: the workspace may come from any earlier solve,
 * however it ended.  The three outputs are zeroed before an argument is refused. */
int dsdf_fem_solve(const DsdfFemOp* op, const double* f, double* u, double rel_tol, int32_t max_iter, int32_t check_every,
                   int32_t* iterations, int32_t* converged, double* ratio, void* ws, size_t ws_bytes, void* stream);
/* we [n_tets]: w_e = lam tr(H)^2 + mu sum_ij H_ij (H_ij + H_ji), H = grad u (StrainEnergyDensityCoefficient.Eval,
 * MFEMLinearElasticity.py:255-266), 0 for a skipped element; wv [n_verts] (NULL with nodal = 0): nodal = 1 the volume-weighted mean
 * over the vertex's elements that count, nodal = 2 the value of the one with the highest index (what ProjectCoefficient, :340, is
 * believed to leave); totals [2] on the device: sum V_e w_e (clcTotCompliance, :371-385) and sum V_e (clcVolume, :387-403). */
int dsdf_fem_energy(const DsdfFemOp* op, const double* u, double* we, int32_t nodal, double* wv, double* totals, void* ws,
                    size_t ws_bytes, void* stream);
/* grad [n_verts][3] = (weight[v], NULL: 1) * sum over the vertex's boundary triangles of (1 / 2) (b - a) x (c - a) / 3: what
 * BoundaryNormalLFIntegrator summed over a P1 space pairs a nodal field with (clcVolumeShapeDerivative, :405-424; with weight = -w_v
 * clcComplianceShapeDerivative, :343-369). */
int dsdf_fem_boundary_gradient(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                               const int64_t* bvstart, const double* weight, double* grad, void* stream);
/* The exact discrete derivative of the compliance with respect to the vertices (numpy restatement:
 * tests/femgrad_numpy.py).  Replaces nothing in the reference, whose clcComplianceShapeDerivative is the boundary formula above.
 * Pi(X, u) = 2 f(X) . u - u^T K(X) u equals the compliance at the solution and is stationary in the free components of u (masked
 * components are zero and stay zero), so d compliance / dX = dPi/dX at fixed u = gK + 2 * sum over the tractions of gL; nodal forces
 * are constants and add nothing.  No new solve.  Additions only: DSDF_ABI_VERSION and dsdf_fem_plan's size and regions are unchanged.
 *
 * Stiffness term.  Per element that counts: H_ij = sum_a u_a,i g_a,j (u as handed in, no mask, as in dsdf_fem_energy),
 *   S = lam tr(H) I + mu (H + H^T), w = lam tr(H)^2 + mu sum_ij H_ij (H_ij + H_ji), E = V (w I - 2 H^T S) with
 *   (H^T S)_kj = sum_i H_ik S_ij (E is not symmetric): d(V w)/dx_b = E g_b, from dV/dx_b = V g_b and
 *   d g_a,j / d x_b,k = -g_b,j g_a,k.  emt [9][n_tets] (the caller's, like we of dsdf_fem_energy) receives E row-major, 3 k + j, in
 *   geom's layout; a skipped element stores nine exact zeros.  grad [n_verts][3]: gK_v = -sum of E_e g_a over the vertex's corners
 *   (e, a) in corner_order's order, at masked vertices too.  u, emt and grad must be three different arrays. */
int dsdf_fem_stiffness_gradient(const DsdfFemOp* op, const double* u, double* emt, double* grad, void* ws, size_t ws_bytes, void* stream);
/* Load term of one traction ([host] 3 finite doubles) on the faces with face_sel[f] != 0 (NULL: all).  Face (a, b, c) in its stored
 *   order: N = (b - a) x (c - a), |N| = sqrt((N.x^2 + N.y^2) + N.z^2), n^ = N / |N|, c_f = ((u~_a + u~_b) + u~_c) . t / 3 with
 *   u~ = u zeroed where mask[v] != 0 (NULL: nowhere), dA_f/dx_a = n^ x (x_c - x_b) / 2, dA_f/dx_b = n^ x (x_a - x_c) / 2,
 *   dA_f/dx_c = n^ x (x_b - x_a) / 2, every operation rounded on its own.  grad [n_verts][3]: gL_v = sum of c_f dA_f/dx_v over the
 *   vertex's boundary corners on selected faces in bcorner_order's order.  A face with |N| == 0 or a non-finite n^ adds exact zeros:
 *   the area is not differentiable there.  u != grad.  Both entries refuse their arguments before any launch. */
int dsdf_fem_load_gradient(const double* verts, int64_t n_verts, const int32_t* bfaces, int64_t n_bfaces, const int64_t* bcorner_order,
                           const int64_t* bvstart, const uint8_t* face_sel, const double* traction, const uint8_t* mask, const double* u,
                           double* grad, void* stream);

/* ---- derivative of a volume mesh with respect to the spline's control points (csrc/voldiff.hpp; fp64 restatement:
 * tests/voldiff_numpy.py).  The reference differentiates its volume mesh through the surface's Jacobian only
 * (analysis/geometry.py:176-197 get_dTheta, from deep_sdf/mesh.py:346-454); here every moving vertex of dsdf_tet_emit's mesh is
 * differentiated in closed form, the face and body diagonals included.  Additions only: DSDF_ABI_VERSION is unchanged.
 *
 * Vertex v = (p, c) = (vert_point[v], vert_class[v]) as dsdf_tet_emit reports it; d = (c & 1, (c >> 1) & 1, (c >> 2) & 1),
 * q = p + sum_b d[b] * stride[b], s0 = grid[p], s1 = grid[q] (the capped grid the mesh was made from).  A class-0 vertex does not
 * move.  For c >= 1 every coordinate b with d[b] = 1 moves by the same t:
 *   d verts[v][b] / d cp[k][l] = d[b] * scale[b] * sum_{e in {0, 1}} dt/ds_e * mask_e * G_e[l] * weight_e(k)
 * with dt/ds_e, the band and its rows exactly dsdf_msd_*'s (above); the band must hold both endpoints of every class >= 1 vertex
 * (an endpoint of a crossing diagonal need not lie on a crossing axis edge: the surface's band is not enough).
 * t_clamp = tau: t = (level - s0) / (s1 - s0) in dsdf_tet_emit's fp32 sequence; when tau > 0 the vertex moves iff
 * tau <= t <= 1 - tau (1 - tau in fp32), i.e. iff the clamp left t unchanged; otherwise its derivative is exactly zero.  tau = 0
 * zeroes nothing.  Both ends are included: t == tau and t == 1 - tau move, one ulp outside is held; a NaN t fails the comparisons
 * and is held when tau > 0.  Inside and outside, ties and non-finite grid values: dsdf_mc_*'s rules ("Ties, zeros, non-finite
 * values").  An endpoint equal to the level gives the OTHER endpoint a factor dt/ds of exactly zero.  A difference s1 - s0 outside
 * fp32's normal range: as for dsdf_msd_* above -- observed behaviour, not a guarantee, except that every other vertex is untouched.
 * The entries work on a compacted list vert_index [n_moving] int32 of ids into the mesh's n_verts vertices (any subset, ascending
 * for a reproducible order; deepsdf_amd passes the class >= 1 vertices): grid vertices, most of a volume mesh, cost nothing.
 * grad_verts / d_verts / normals are [n_verts][3] and are addressed through vert_index.  A list entry outside 0 .. n_verts - 1, a
 * class outside 1 .. 7, a point outside the grid, a far endpoint past the grid, a band row or base out of range contributes
 * nothing; nothing is read or written out of bounds for in-range arrays.
 *   dsdf_vd_jvp     d_cp [ncp][L] -> d_verts [n_verts][3]: the entry zeroes all of d_verts, then one wave per list entry writes
 *                   its row: coordinate b = fma(scale[b] * dt1, dot1, fma(scale[b] * dt0, dot0, 0)) where d[b] = 1 (dot_e: the
 *                   endpoint's (slot, l) products over the lanes and a fixed xor-shuffle tree, as dsdf_msd_jvp), 0 elsewhere.  A
 *                   class-1/2/4 vertex has dsdf_msd_jvp's bits.
 *   dsdf_vd_vjp     grad_verts [n_verts][3] -> grad_cp [ncp][L].  Per list entry gs = sum over b with d[b] = 1, in increasing b,
 *                   of scale[b] * grad_verts[v][b] (every product and sum rounded on its own); endpoint e adds
 *                   fma(gs * dt_e, weight * G[l], acc).  Two stages as dsdf_msd_vjp: ceil(n_moving / 512) partial sums in list
 *                   order, then their sum in part order; ws from dsdf_vd_vjp_workspace_bytes (256-byte aligned, planner
 *                   conventions, region vd_vjp_part).
 *   dsdf_vd_dtheta  out [n_moving][3][R], R = ncp * L: the reference's get_dTheta (analysis/geometry.py:176-197: stretch,
 *                   jac[jac > 1] = 0, jac[jac < -1] = 0, dot_prod with the normal) for list entry i, normal n = normals[v],
 *                   column r = (k, l), fp32, every operation rounded once:
 *                     T    = (0 + (dt0 * weight0(k)) * G0[l]) + (dt1 * weight1(k)) * G1[l]   (no fused multiply-add; an endpoint
 *                            that contributes nothing, or whose support does not hold k, is left out)
 *                     j[b] = (stretch[b] * scale[b]) * T where d[b] = 1, 0 elsewhere; if clip > 0 and |j[b]| > clip: j[b] = 0
 *                     nj   = ((0 + n[0] j[0]) + n[1] j[1]) + n[2] j[2],   nn = (n[0] n[0] + n[1] n[1]) + n[2] n[2]
 *                     out[i][b][r] = n[b] * (nj / nn);  a vertex with nn = 0 or one that does not move: +0.
 *                   dsdf_mt_project's rule carried to several coordinates.  stretch [host] 3 floats.
 * No atomics; two identical calls give identical bytes.  Every argument error returns DSDF_E_INVALID before anything is launched. */
typedef struct DsdfVdMesh {
  const float* grid;               /* device, capped sdf [dims[0]][dims[1]][dims[2]] */
  const int64_t* vert_point;       /* device [n_verts] */
  const int32_t* vert_class;       /* device [n_verts] */
  const int32_t* vert_index;       /* device [n_moving] */
  const int32_t* band_of;          /* device [grid points]: band row of a grid index, < 0: none */
  int64_t n_verts, n_moving;
  int32_t dims[3];                 /* 2 .. 1024 */
  float scale[3];                  /* voxel_size / 2 of the returned vertices */
  float level;
  float t_clamp;                   /* dsdf_tet_emit's, [0, 0.5) */
} DsdfVdMesh;

int dsdf_vd_vjp_workspace_bytes(int64_t n_moving, int64_t n_control_points, int32_t L, size_t* bytes, int32_t* n_parts); /* [host] */
int dsdf_vd_jvp(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* d_cp, float* d_verts, void* stream);
int dsdf_vd_vjp(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* grad_verts, float* grad_cp, void* ws,
                size_t ws_bytes, void* stream);
int dsdf_vd_dtheta(const DsdfVdMesh* mesh, const DsdfMsdBand* band, const float* normals, const float* stretch /*[host]*/,
                   float clip, float* out, void* stream);

/* ---- building blocks (exported for the parity tests and profiling; not needed by a trainer) --------- */
/* C[M,N] = A[M,K] * B[N,K]^T (+bias) */
int dsdf_gemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                 int64_t N, int64_t K, const float* bias, void* stream);
/* C[M,N] = A[K,M]^T * B[K,N]  (split-K inside; ws holds the partial slabs).  ldc == N <= 2048.  ws: nsplit slabs of
 * rup(M * ldc, 64) floats, nsplit = ceil(K / kchunk), kchunk = rup(ceil(K / min(32, ceil(K / 256))), 32), and M floats behind
 * them (+ one debug red zone behind each of the two when dsdf_debug_ws_redzone is set). */
int dsdf_gemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M,
                 int64_t N, int64_t K, void* ws, size_t ws_bytes, void* stream);
/* keep-mask of the dropout hash as 0/1 bytes [rows, cols] (spec: oracle/deepsdf_oracle.py dropout_keep) */
int dsdf_dropout_mask(uint32_t key, float p, int64_t rows, int64_t cols, int64_t row_offset, uint8_t* out,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DSDF_H */
