/*
 * vunet_seq_cls.h -- C ABI of the real-vs-fake classifier study of run_inference (csrc/seq_cls.hip).  Part of libvunet_hip.so;
 * same conventions as vunet_hip.h (plain pointers and sizes, caller-owned fp32 device buffers, `stream` = hipStream_t as
 * void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   models/pose_behavior_rnn.py:6-17        Classifier(51, 1): nn.GRU(51, 256, batch_first) -> h_T -> nn.Linear(256, 1)
 *   models/pose_behavior_rnn.py:33-44       Regressor(H, 51): fc3(relu(fc2(relu(fc1(mu)))))
 *   experiments/behavior_net.py:1315-1521   per start time: SGD(lr 1e-3, momentum 0.9) on BCEWithLogits(fake -> 0, real -> 1),
 *                                           Adam(lr 1e-3) on mean_rows ||regressor(mu) - x[:, start]||
 *
 * Every launch covers a set of independent NETS ("nets" = grid y); a net's arithmetic never depends on how many share the
 * launch.  Nothing is an atomic; every sum has a fixed order.  Which batch a launch reads comes from a device-resident
 * iteration counter (it_dev: batch = *it_dev % nb), advanced by vunet_seq_cls_tick, so a recorded hipGraph replays the study.
 *
 * A classifier's parameters are one block of VUNET_CLS_P floats, in torch's gate order r, z, n:
 *   [0, OFF_WHH)        weight_ih_l0 [768][64]  (51 columns used, 52 .. 63 zero)
 *   [OFF_WHH, OFF_BIH)  weight_hh_l0 [768][256]
 *   [OFF_BIH, OFF_BHH)  bias_ih_l0 [768];  [OFF_BHH, OFF_FCW) bias_hh_l0 [768]
 *   [OFF_FCW, OFF_FCB)  fc1.weight [256];  OFF_FCB fc1.bias
 * Gradients: S split slices of that block per net ([nets][S][P]); the matrices and GRU biases are summed over the slices, the
 * head's two fc entries are read from slice 0.
 */
#ifndef VUNET_SEQ_CLS_H
#define VUNET_SEQ_CLS_H
#include <stddef.h>
#include <stdint.h>

#include "vunet_seq_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_CLS_NIN 51
#define VUNET_CLS_KP 64
#define VUNET_CLS_H 256
#define VUNET_CLS_G 768
#define VUNET_CLS_OFF_WHH (VUNET_CLS_G * VUNET_CLS_KP)
#define VUNET_CLS_OFF_BIH (VUNET_CLS_OFF_WHH + VUNET_CLS_G * VUNET_CLS_H)
#define VUNET_CLS_OFF_BHH (VUNET_CLS_OFF_BIH + VUNET_CLS_G)
#define VUNET_CLS_OFF_FCW (VUNET_CLS_OFF_BHH + VUNET_CLS_G)
#define VUNET_CLS_OFF_FCB (VUNET_CLS_OFF_FCW + VUNET_CLS_H)
#define VUNET_CLS_P (VUNET_CLS_OFF_FCB + 4)
#define VUNET_CLS_MAX_BS 1024

/* C[net][s][m][n] (=, or += with accumulate) sum_{k in split s} A[m][k] B[k][n] (+ bias[n] where s == 0), then ReLU (relu != 0)
 * and / or times [mask[m][n] > 0] (mask != NULL).  Every operand is addressed by element strides, so transposes are strides;
 * a zero stride broadcasts (B = a single 1.0 with b_k = b_n = 0 sums the rows of A).  Split s covers
 * k in [s Kc, min(K, (s + 1) Kc)), Kc = ceil(K / split) rounded up to 4; its result goes to C + s c_split.
 * Exact fp32 on v_mfma_f32_16x16x4_f32: one 64-lane workgroup per 32 x 32 tile of C, k ascending. */
typedef struct vunet_seq_cls_gemm {
  const float* A;
  const float* B;
  float* C;
  const float* bias;
  const float* mask;
  int64_t a_net, a_m, a_k;
  int64_t b_net, b_k, b_n;
  int64_t c_net, c_m, c_n, c_split;
  int64_t bias_net, mask_net, mask_m;
  int32_t M, N, K, nets, split, relu, accumulate, pad;
} vunet_seq_cls_gemm;
int vunet_seq_cls_gemm_run(const vunet_seq_cls_gemm* d, void* stream);

/* Rows of the batch b = *it_dev % nb.  For net g (src_dev: a device table of 2 nets pointers: fake set, real set or NULL) and
 * r < R (R = bs without a real set, 2 bs with one): dst[g][t][r][k] = set[b bs + r % bs][t][k] (fake for r < bs, real after),
 * k < n; 0 for n <= k < ld.  Sets are [N][T][n]; dst net stride dst_net. */
int vunet_seq_cls_gather(const float* const* src_dev, int32_t nets, int32_t T, int32_t n, int32_t ld, int32_t bs, int32_t nb,
                         int32_t with_real, const int32_t* it_dev, float* dst, int64_t dst_net, void* stream);

/* The GRU cell of step t for R rows (torch.nn.GRU, gate order r, z, n):  gi = x W_ih^T + b_ih, gh = h W_hh^T + b_hh,
 *   r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = n + z (h - n).
 * gi, gh, gates: [T][R][768] per net (gates keeps r | z | n), h: [T + 1][R][256] per net (h_0 = 0 is the caller's);
 * net strides gi_net / h_net (the same for gh and gates as for gi). */
int vunet_seq_cls_cell_fwd(const float* gi, const float* gh, float* gates, float* h, int32_t nets, int32_t T, int32_t R, int32_t t,
                           int64_t gi_net, int64_t h_net, void* stream);

/* Head and loss: logit[r] = fc1.w . h_T[r] + fc1.b.  Fake rows r < bs (target 0), real rows bs <= r < 2 bs (with_real).
 * loss = mean_fake BCE(logit, 0) + mean_real BCE(logit, 1) -> loss_out[g][*it_dev + slot_off] (with_real);
 * acc = mean_fake sigmoid(logit) -> acc_out[g][*it_dev + slot_off].  Curves: ld_curve floats per net.
 * dh != NULL (training): dh[g][r][j] = dlogit[r] fc1.w[j] and the fc1 gradients -> grad[g][OFF_FCW ..] (slice 0). */
int vunet_seq_cls_head(const float* hT, int64_t h_net, const float* params, int32_t nets, int32_t bs, int32_t with_real,
                       const int32_t* it_dev, int32_t slot_off, float* loss_out, float* acc_out, int32_t ld_curve, float* dh,
                       float* grad, int64_t grad_net, void* stream);

/* Back through the cell of step t: dh (dL/dh_{t+1}, [R][256] per net, net stride dh_net) ->
 *   dgi[t] = (da_r, da_z, da_n) written over gi[t];  dgh[t] = (da_r, da_z, da_n r) written over gh[t] (gh_n read first);
 *   dh_prev = dh z (the product dgh . W_hh is added by vunet_seq_cls_gemm_run with accumulate). */
int vunet_seq_cls_cell_bwd(float* gi, float* gh, const float* gates, const float* h, const float* dh, float* dh_prev, int32_t nets,
                           int32_t T, int32_t R, int32_t t, int64_t gi_net, int64_t h_net, int64_t dh_net, void* stream);

/* torch.optim.SGD(lr, momentum) on the parameter blocks: g = the summed gradient slices; buf = g on the first iteration
 * (*it_dev == 0), else momentum buf + g; p -= lr buf.  params, buf: [nets][P]; grad: [nets][S][P]. */
int vunet_seq_cls_sgd(float* params, const float* grad, float* buf, int32_t nets, int32_t S, float lr, float momentum,
                      const int32_t* it_dev, void* stream);

/* The regressor's loss (one workgroup per net): target = xo[b bs + r][start_dev[g]] (xo [N][T][51], b = *it_dev % nb);
 * d_r = ||pred[r] - target||, loss = mean_r d_r -> loss_out[g][*it_dev + slot_off]; dpred = (pred - target) / (d_r bs) (0 where
 * d_r == 0).  xc != NULL: de = mean_r ||xc[b bs + r][start] - target|| -> de_out[g][*it_dev + slot_off].
 * pred and dpred: [bs][ldp] per net; columns 51 .. ldp of pred are not read and those of dpred are not written (they keep
 * what the caller put there). */
int vunet_seq_cls_reg_loss(const float* pred, int32_t ldp, int64_t pred_net, const float* xo, const float* xc, int32_t T, int32_t bs,
                           int32_t nb, const int32_t* start_dev, const int32_t* it_dev, int32_t slot_off, float* loss_out,
                           float* de_out, int32_t ld_curve, float* dpred, int32_t nets, void* stream);

/* torch.optim.Adam (defaults but lr) on n contiguous floats per net: p, m, v, g with net stride n.  beta1 / beta2 outside
 * [0, 1) and eps < 0 are refused, as vunet_seq_reg_fc4_adam refuses them. */
int vunet_seq_cls_adam(float* p, float* m, float* v, const float* g, int32_t nets, int64_t n, const vunet_seq_adam_hp* hp, void* stream);

/* One thread: *it_dev += 1 (it_dev != NULL), *step_dev += 1 (step_dev != NULL). */
int vunet_seq_cls_tick(int32_t* it_dev, int64_t* step_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
