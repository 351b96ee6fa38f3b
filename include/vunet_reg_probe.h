/*
 * vunet_reg_probe.h -- C ABI of the image experiments' post-hoc pose-regressor probe, csrc/reg_probe.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned fp32 device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   models/vunets.py:786-824                     Regressor: pred = linears(cat(relu(embedder_e(latent_e))))
 *   experiments/shape_and_pose_net.py:921-995    run_inference's probe: 20 epochs of Adam(lr=0.001) on
 *   experiments/vunet.py:745-805                 loss = mean_b ||pred_b - kps_b||_2 with the VUnet frozen
 *
 * One training step (rows padded to Bp = 16 ceil(B / 16), B <= 64; all matrices row-major fp32):
 *   forward    vunet_reg_probe_embed + vunet_reg_probe_embed_finish per embedder (a full-window valid convolution is the
 *              linear map W[out][in k k] of the flattened latent: the state-dict tensor IS that matrix), into the concat
 *              operand of the first linear layer; vunet_seq_linear (vunet_hip.h; ReLU: act 3) for the linears
 *   loss       vunet_reg_probe_loss
 *   dX         vunet_seq_dx / vunet_seq_dz_finish (slope 0) down to the embedders' outputs (vunet_seq_train.h); the embedders
 *              need no input gradient
 *   update     vunet_seq_adam_tick; vunet_seq_dw over every layer: dW fused into torch.optim.Adam's update
 */
#ifndef VUNET_REG_PROBE_H
#define VUNET_REG_PROBE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Split-K product of a wide-K, narrow-output layer: part[s][b][m] = sum over k in slab s of w[m][k] x[b][k].
 * x: [Bp][K] (rows B .. Bp zero), w: [>= M][K], part: [S][Bp][M] RAW partial slabs; slab s is k in [s K / S, (s + 1) K / S).
 * M % 16 == 0, K % (64 S) == 0, 1 <= B <= 64.  A workgroup owns one 16-row tile of w over one slab; v_mfma_f32_16x16x4_f32
 * (exact fp32); a wave adds its chunks in ascending k, the four waves are added in wave order: bit-reproducible, no atomics. */
int vunet_reg_probe_embed(const float* x, const float* w, int32_t B, int32_t M, int32_t K, int32_t S, float* part, void* stream);

/* y[b][col_off + m] = max(sum_s part[s][b][m] + bias[m], 0), slabs in order, for b < B; rows B .. Bp of those M columns: 0.
 * y: [Bp][ldy]; M % 16 == 0, ldy % 4 == 0, col_off % 4 == 0, col_off + M <= ldy.  Columns outside [col_off, col_off + M) are
 * not written. */
int vunet_reg_probe_embed_finish(const float* part, int32_t S, const float* bias, int32_t B, int32_t M, float* y, int32_t ldy,
                                 int32_t col_off, void* stream);

/* loss = (1 / B) sum_{b < B} ||pred_b - tgt_b||_2 over n columns (pred: [Bp][ldp], tgt: [B][ldt]);
 * dpred[b][d] = (pred - tgt) / (B ||.||_2), 0 for a row of norm 0 (torch's norm backward) and on padded rows and columns
 * ([Bp][ldp], all written).  last[0] = loss.  losses != NULL: i = *cursor; losses[i] = loss if i < cap; *cursor = i + 1 -- the
 * loss course stays on the device, a recorded step appends to it at every replay.  One workgroup. */
int vunet_reg_probe_loss(const float* pred, int32_t ldp, const float* tgt, int32_t ldt, int32_t B, int32_t n, float* dpred,
                         float* last, float* losses, int32_t cap, int32_t* cursor, void* stream);

#ifdef __cplusplus
}
#endif
#endif
