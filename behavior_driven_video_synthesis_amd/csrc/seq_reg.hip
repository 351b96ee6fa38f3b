// The adversarial pose regressor of the behaviour cVAE's step (BASELINE config 4 with ``use_regressor``: experiments/
// behavior_net.py:627-648, models/pose_behavior_rnn.py:47-62).  Interface: include/vunet_seq_reg.h.
//
// The regressor's matrix work runs on the seq family's kernels -- vunet_seq_linear (ReLU: act 3), vunet_seq_dx,
// vunet_seq_dz_finish (slope 0) and the weight-gradient sweep fused into Adam, vunet_seq_dw -- all exact fp32 on
// v_mfma_f32_16x16x4_f32.  What is here is the part those do not cover:
//   * seq_reg_gather_kernel: fc4 of a one-hot is one column of W4 plus b4, the same for every row: it is read, not multiplied,
//     at the index the step drew (device memory: a recorded hipGraph replays with fresh indices), and written with fc3's
//     output into the concat operand of fc5; the same launch gathers the target rows seq_b[:, idx].
//   * seq_reg_loss_kernel: the mean squared error, its gradient, and after the fifth inner step the clamp coefficient of the
//     adversarial term and that term's share of the logged loss.
//   * seq_reg_cat_bwd_kernel: fc5's input gradient (raw slabs) split at the concat, through ReLU'.
//   * seq_reg_fc4_adam_kernel: Adam on fc4 with the one-column gradient formed inside the update (no dense dW4).
//   * seq_reg_adv_kernel: the adversarial gradient wrt mu, added into the cVAE loss's d loss / d mu.
// Nothing uses float atomics; every sum has a fixed order.
#include "common.h"
#include "../../include/vunet_seq_reg.h"
#include "seq_adam.h"

namespace {

__global__ __launch_bounds__(256) void seq_reg_gather_kernel(const float* __restrict__ w4, const float* __restrict__ b4,
                                                             const int32_t* __restrict__ idx_dev, int k, const float* __restrict__ h3,
                                                             const float* __restrict__ seq, int seq_stride, int n, int B, int H4,
                                                             float* __restrict__ cat, float* __restrict__ tgt) {
  const int b = blockIdx.x, K5 = H4 + VUNET_SEQ_REG_C;
  int idx = idx_dev[k];
  idx = idx < 0 ? 0 : (idx >= VUNET_SEQ_REG_T ? VUNET_SEQ_REG_T - 1 : idx);   // (the host draws / checks [0, 50))
  for (int j = threadIdx.x; j < H4; j += 256) cat[(size_t)b * K5 + j] = h3[(size_t)b * H4 + j];
  for (int c = threadIdx.x; c < VUNET_SEQ_REG_C; c += 256)
    cat[(size_t)b * K5 + H4 + c] = fmaxf(w4[c * VUNET_SEQ_REG_T + idx] + b4[c], 0.f);
  for (int d = threadIdx.x; d < n; d += 256) tgt[(size_t)b * n + d] = b < B ? seq[(size_t)b * seq_stride + (size_t)idx * n + d] : 0.f;
}

__global__ __launch_bounds__(256) void seq_reg_loss_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ tgt, int B,
                                                           int Bp, int n, int k, float w, float* __restrict__ reg,
                                                           float* __restrict__ dpred, float* __restrict__ scalars) {
  __shared__ float red[4];
  const float scale = 2.f / ((float)B * (float)n);
  float s = 0.f;
  for (int e = threadIdx.x; e < Bp * ldp; e += 256) {
    const int b = e / ldp, d = e - b * ldp;
    float g = 0.f;
    if (b < B && d < n) {
      const float r = pred[e] - tgt[(size_t)b * n + d];
      s += r * r;
      g = scale * r;
    }
    dpred[e] = g;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x) return;
  const float L = ((red[0] + red[1]) + (red[2] + red[3])) / ((float)B * (float)n);
  reg[k] = L;
  if (scalars) {   // loss -= clamp(L, max=0.45) w;  loss -= clamp(L, max=0.7) w   (experiments/behavior_net.py:647-648)
    reg[5] = -w * ((L <= 0.45f ? 1.f : 0.f) + (L <= 0.7f ? 1.f : 0.f));
    float loss = scalars[0];
    loss -= fminf(L, 0.45f) * w;
    loss -= fminf(L, 0.7f) * w;
    scalars[0] = loss;
  }
}

__global__ __launch_bounds__(256) void seq_reg_cat_bwd_kernel(const float* __restrict__ raw, int S, int Bp, int H4,
                                                              const float* __restrict__ cat, float* __restrict__ dz3, float* __restrict__ dzc) {
  const int K5 = H4 + VUNET_SEQ_REG_C;
  const size_t per = (size_t)Bp * K5, e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= per) return;
  float v = raw[e];
  for (int s = 1; s < S; ++s) v += raw[(size_t)s * per + e];
  v *= cat[e] > 0.f ? 1.f : 0.f;   // ReLU' read off the saved output
  const int b = (int)(e / K5), c = (int)(e - (size_t)b * K5);
  if (c < H4) dz3[(size_t)b * H4 + c] = v;
  else if (dzc) dzc[(size_t)b * VUNET_SEQ_REG_C + c - H4] = v;
}

// one wave per row c of W4: the column sum of dzc over the batch, then Adam on the row's 50 weights and its bias
__global__ __launch_bounds__(64) void seq_reg_fc4_adam_kernel(const float* __restrict__ dzc, int Bp, const int32_t* __restrict__ idx_dev,
                                                              int k, float* __restrict__ w4, float* __restrict__ b4, float* __restrict__ m4,
                                                              float* __restrict__ v4, float* __restrict__ bm4, float* __restrict__ bv4,
                                                              vunet_seq_adam_hp hp) {
  const int c = blockIdx.x, lane = threadIdx.x;
  int idx = idx_dev[k];
  idx = idx < 0 ? 0 : (idx >= VUNET_SEQ_REG_T ? VUNET_SEQ_REG_T - 1 : idx);   // the column seq_reg_gather_kernel read
  const AdamResolved h = adam_resolve(hp);
  const float g = wave_sum(lane < Bp ? dzc[(size_t)lane * VUNET_SEQ_REG_C + c] : 0.f);
  if (lane < VUNET_SEQ_REG_T) {
    const size_t o = (size_t)c * VUNET_SEQ_REG_T + lane;
    float p = w4[o], m = m4[o], v = v4[o];
    adam_update(h, lane == idx ? g : 0.f, p, m, v);
    w4[o] = p;
    m4[o] = m;
    v4[o] = v;
  }
  if (lane == 0) {
    float p = b4[c], m = bm4[c], v = bv4[c];
    adam_update(h, g, p, m, v);
    b4[c] = p;
    bm4[c] = m;
    bv4[c] = v;
  }
}

__global__ __launch_bounds__(256) void seq_reg_adv_kernel(const float* __restrict__ raw, int S, int B, int Bp, int H,
                                                          const float* __restrict__ reg, float* __restrict__ gmu, float* __restrict__ adv) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)B * H) return;
  const size_t per = (size_t)Bp * H;
  float v = raw[e];
  for (int s = 1; s < S; ++s) v += raw[(size_t)s * per + e];
  v *= reg[5];
  gmu[e] += v;
  if (adv) adv[e] = v;
}

}  // namespace

extern "C" int vunet_seq_reg_gather(const float* w4, const float* b4, const int32_t* idx_dev, int32_t k, const float* h3, const float* seq,
                                    int32_t seq_stride, int32_t n, int32_t B, int32_t H4, float* cat, float* tgt, void* stream) {
  if (!w4 || !b4 || !idx_dev || !h3 || !seq || !cat || !tgt || k < 0 || k > 4 || n < 1 || B < 1 || B > 64 || H4 < 1) return VUNET_ERR_ARG;
  if (seq_stride < VUNET_SEQ_REG_T * n) return VUNET_ERR_ARG;
  const int Bp = (B + 15) / 16 * 16;
  VUNET_LAUNCH(seq_reg_gather_kernel, dim3(Bp), dim3(256), 0, (hipStream_t)stream, w4, b4, idx_dev, k, h3, seq, seq_stride, n, B, H4, cat,
               tgt);
  return vunet_check_launch();
}

extern "C" int vunet_seq_reg_loss(const float* pred, int32_t ldp, const float* tgt, int32_t B, int32_t n, int32_t k, float w, float* reg,
                                  float* dpred, float* scalars, void* stream) {
  if (!pred || !tgt || !reg || !dpred || B < 1 || B > 64 || n < 1 || ldp < n || k < 0 || k > 4) return VUNET_ERR_ARG;
  const int Bp = (B + 15) / 16 * 16;
  VUNET_LAUNCH(seq_reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, ldp, tgt, B, Bp, n, k, w, reg, dpred, scalars);
  return vunet_check_launch();
}

extern "C" int vunet_seq_reg_cat_bwd(const float* raw, int32_t S, int32_t Bp, int32_t H4, const float* cat, float* dz3, float* dzc,
                                     void* stream) {
  if (!raw || !cat || !dz3 || S < 1 || Bp < 16 || Bp > 64 || Bp % 16 || H4 < 1) return VUNET_ERR_ARG;
  const size_t per = (size_t)Bp * (H4 + VUNET_SEQ_REG_C);
  VUNET_LAUNCH(seq_reg_cat_bwd_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw, S, Bp, H4, cat, dz3,
               dzc);
  return vunet_check_launch();
}

extern "C" int vunet_seq_reg_fc4_adam(const float* dzc, int32_t Bp, const int32_t* idx_dev, int32_t k, float* w4, float* b4, float* m4,
                                      float* v4, float* bm4, float* bv4, const vunet_seq_adam_hp* hp, void* stream) {
  if (!dzc || !idx_dev || !w4 || !b4 || !m4 || !v4 || !bm4 || !bv4 || !hp || Bp < 16 || Bp > 64 || Bp % 16 || k < 0 || k > 4)
    return VUNET_ERR_ARG;
  if (!hp->lr_dev || !hp->step_dev || hp->beta1 < 0.f || hp->beta1 >= 1.f || hp->beta2 < 0.f || hp->beta2 >= 1.f || hp->eps < 0.f)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(seq_reg_fc4_adam_kernel, dim3(VUNET_SEQ_REG_C), dim3(64), 0, (hipStream_t)stream, dzc, Bp, idx_dev, k, w4, b4, m4, v4, bm4,
               bv4, *hp);
  return vunet_check_launch();
}

extern "C" int vunet_seq_reg_adv(const float* raw, int32_t S, int32_t B, int32_t H, const float* reg, float* gmu, float* adv, void* stream) {
  if (!raw || !reg || !gmu || S < 1 || B < 1 || B > 64 || H < 1) return VUNET_ERR_ARG;
  const int Bp = (B + 15) / 16 * 16;
  const size_t n = (size_t)B * H;
  VUNET_LAUNCH(seq_reg_adv_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, raw, S, B, Bp, H, reg, gmu, adv);
  return vunet_check_launch();
}
