/*
 * vunet_seq_reg.h -- C ABI of the behaviour cVAE's adversarial pose regressor and its KL-weight variant (BASELINE config 4,
 * ``use_regressor`` / ``cvae``), csrc/seq_reg.hip and csrc/seq_bptt.hip.  Part of libvunet_hip.so; same conventions as
 * vunet_hip.h (plain pointers and sizes, caller-owned fp32 device buffers, `stream` = hipStream_t as void*, 0 or a negative
 * VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   models/pose_behavior_rnn.py:47-62        Regressor_fly: pred = fc5([relu(fc3(relu(fc2(relu(fc1(mu)))))) | relu(fc4(onehot))])
 *   experiments/behavior_net.py:305-306      Adam(regressor.parameters(), lr=1e-4)
 *   experiments/behavior_net.py:627-648      five inner steps: idx ~ U[0, T); L = mean((pred - seq_b[:, idx])^2); backward; Adam;
 *                                            then loss -= w clamp(L_5, max=0.45) + w clamp(L_5, max=0.7)
 *   experiments/behavior_net.py:606-611      tuning = 1 if cvae else gamma
 *
 * One inner step k (H = dim_hidden_b, H4 = H / 4, K5 = H4 + 128, rows padded to Bp = 16 ceil(B / 16)):
 *   forward    vunet_seq_linear (act 3, ReLU) fc1 -> fc2 -> fc3; vunet_seq_reg_gather (fc4 on the one-hot, the concat operand of
 *              fc5, the target row); vunet_seq_linear fc5 (its 51 rows padded to 64)
 *   loss       vunet_seq_reg_loss       L_k and d L_k / d pred
 *   dX         vunet_seq_dx fc5 -> vunet_seq_reg_cat_bwd -> vunet_seq_dx fc3 -> vunet_seq_dz_finish (slope 0) -> ... -> dZ of fc1,
 *              all on the weights before this step's update
 *   update     vunet_seq_adam_tick; vunet_seq_dw (fc1, fc2, fc3, fc5: dW fused into Adam); vunet_seq_reg_fc4_adam
 * After the fifth: the same dX chain on the UPDATED weights with the fifth forward's ReLU masks -- what torch 1.3.1 computes,
 * whose Adam writes through p.data -- down to mu, scaled by the clamp coefficient: vunet_seq_reg_adv.
 */
#ifndef VUNET_SEQ_REG_H
#define VUNET_SEQ_REG_H
#include <stddef.h>
#include <stdint.h>

#include "vunet_seq_train.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fc4 is Linear(50, 128): the one-hot's width is the sequence length the regressor was built for */
#define VUNET_SEQ_REG_T 50
#define VUNET_SEQ_REG_C 128

/* idx = idx_dev[k] (clamped into [0, 50)).  For every padded row b < Bp:
 *   cat[b][j] = h3[b][j] (j < H4);  cat[b][H4 + c] = max(w4[c][idx] + b4[c], 0)   (fc4 of the one-hot: column idx of W4, c < 128)
 *   tgt[b][d] = seq[b seq_stride + idx n + d] (b < B; rows B .. Bp: 0)              (seq_b[:, idx]) */
int vunet_seq_reg_gather(const float* w4, const float* b4, const int32_t* idx_dev, int32_t k, const float* h3, const float* seq,
                         int32_t seq_stride, int32_t n, int32_t B, int32_t H4, float* cat, float* tgt, void* stream);

/* L = mean over b < B, d < n of (pred[b][d] - tgt[b][d])^2 -> reg[k];  dpred[b][d] = 2 (pred - tgt) / (B n), 0 on padded rows and
 * columns (d in [n, ldp)).  scalars != NULL (the fifth step): reg[5] = -w ([L <= 0.45] + [L <= 0.7]) (clamp's backward keeps the
 * boundary) and scalars[0] = (scalars[0] - w min(L, 0.45)) - w min(L, 0.7).  reg: [6] floats.  One workgroup. */
int vunet_seq_reg_loss(const float* pred, int32_t ldp, const float* tgt, int32_t B, int32_t n, int32_t k, float w, float* reg,
                       float* dpred, float* scalars, void* stream);

/* The input gradient of fc5 split at the concat: v[b][c] = (sum_s raw[s][b][c]) (cat[b][c] > 0), slabs in order ([S][Bp][K5] from
 * vunet_seq_dx).  dz3[b][j] = v[b][j] (j < H4, [Bp][H4]);  dzc[b][c] = v[b][H4 + c] ([Bp][128]; NULL: not wanted). */
int vunet_seq_reg_cat_bwd(const float* raw, int32_t S, int32_t Bp, int32_t H4, const float* cat, float* dz3, float* dzc, void* stream);

/* Adam on fc4 (w4 [128][50], b4 [128]) with its gradient formed in place: g[c] = sum_{b < Bp} dzc[b][c] (batch order) is the
 * bias gradient and column idx_dev[k] (clamped into [0, 50), as vunet_seq_reg_gather reads it) of the weight gradient; every
 * other column's gradient is 0 (Adam still moves it).  beta1 / beta2 outside [0, 1) and eps < 0 are refused. */
int vunet_seq_reg_fc4_adam(const float* dzc, int32_t Bp, const int32_t* idx_dev, int32_t k, float* w4, float* b4, float* m4, float* v4,
                           float* bm4, float* bv4, const vunet_seq_adam_hp* hp, void* stream);

/* The adversarial term's gradient wrt mu: a[b][j] = reg[5] sum_s raw[s][b][j] ([S][Bp][H] from vunet_seq_dx over fc1), b < B:
 * gmu[b][j] += a[b][j];  adv != NULL: adv[b][j] = a[b][j] as well. */
int vunet_seq_reg_adv(const float* raw, int32_t S, int32_t B, int32_t H, const float* reg, float* gmu, float* adv, void* stream);

/* vunet_seq_vae_loss with the KL term weighted by *kl_weight_dev instead of gamma (``cvae: True``: 1); gamma still advances
 * (gamma_step > 0) as the controller does, from the step's kl.  scalars[3] = the weight used.  Other arguments and outputs as
 * vunet_seq_vae_loss (include/vunet_seq_train.h). */
int vunet_seq_vae_loss_w(const float* xs, const float* target, const float* mu, const float* logstd, int32_t B, int32_t T, int32_t n,
                         int32_t H, float recon_weight, const float* kl_weight_dev, float* gamma_dev, const float* imax_dev,
                         float gamma_step, float* part, float* scalars, float* per_seq, float* dxs, float* dmu, float* dlogstd,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
