// The real-vs-fake classifier study of run_inference (experiments/behavior_net.py:1302-1521): GRU classifiers
// (models/pose_behavior_rnn.py:6-17) trained with SGD-momentum, and the mu -> pose regressor (:33-44) trained with Adam, for
// every start time at once.  Interface: include/vunet_seq_cls.h.
//
// Every matrix product -- the input projection of all T steps, the recurrent product of each step, dh_{t-1} = dgh . W_hh, the
// weight and bias gradients reduced over all steps and rows, and the regressor's three layers forward and backward -- is one
// strided batched kernel, cls_gemm_kernel: a 64-lane workgroup per 32 x 32 tile of C, exact fp32 on v_mfma_f32_16x16x4_f32
// with k ascending, its nets on grid y and its K splits on grid z (slices summed in slice order by whoever reads them).  The
// elementwise work between products is here too: the GRU cell forward and backward, the head with BCEWithLogits, SGD with
// momentum, the regressor's norm loss, Adam (seq_adam.h), and the iteration counter.  Nothing uses atomics.
#include "common.h"
#include "../../include/vunet_seq_cls.h"
#include "seq_adam.h"

namespace {

__global__ __launch_bounds__(64) void cls_gemm_kernel(vunet_seq_cls_gemm d) {
  const int tiles_n = (d.N + 31) / 32;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int net = blockIdx.y, s = blockIdx.z;
  const int m0 = tm * 32, n0 = tn * 32;
  const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
  const int kc = ((d.K + d.split - 1) / d.split + 3) & ~3;
  const int kb = s * kc, ke = min(d.K, kb + kc);
  const float* A = d.A + net * d.a_net;
  const float* B = d.B + net * d.b_net;
  const bool am0 = m0 + li < d.M, am1 = m0 + 16 + li < d.M, bn0 = n0 + li < d.N, bn1 = n0 + 16 + li < d.N;
  const int64_t ao0 = (int64_t)(m0 + li) * d.a_m, ao1 = (int64_t)(m0 + 16 + li) * d.a_m;
  const int64_t bo0 = (int64_t)(n0 + li) * d.b_n, bo1 = (int64_t)(n0 + 16 + li) * d.b_n;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int k = kb; k < ke; k += 4) {
    const int kk = k + lk;
    const bool kin = kk < ke;
    const int64_t ak = (int64_t)kk * d.a_k, bk = (int64_t)kk * d.b_k;
    const float a0 = (kin && am0) ? A[ao0 + ak] : 0.f;
    const float a1 = (kin && am1) ? A[ao1 + ak] : 0.f;
    const float b0 = (kin && bn0) ? B[bk + bo0] : 0.f;
    const float b1 = (kin && bn1) ? B[bk + bo1] : 0.f;
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
  float* C = d.C + net * d.c_net + s * d.c_split;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + 16 * j + li;
    if (n >= d.N) continue;
    const float bias = (d.bias && s == 0) ? d.bias[net * d.bias_net + n] : 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = m0 + 16 * i + 4 * lk + v;
        if (m >= d.M) continue;
        float* c = C + (int64_t)m * d.c_m + (int64_t)n * d.c_n;
        float r = acc[i][j][v] + bias;
        if (d.accumulate) r = *c + r;
        if (d.relu) r = fmaxf(r, 0.f);
        if (d.mask) r = d.mask[net * d.mask_net + (int64_t)m * d.mask_m + n] > 0.f ? r : 0.f;
        *c = r;
      }
  }
}

__global__ __launch_bounds__(256) void cls_gather_kernel(const float* const* __restrict__ src, int T, int n, int ld, int bs, int nb,
                                                         int with_real, const int32_t* __restrict__ it_dev, float* __restrict__ dst,
                                                         int64_t dst_net) {
  const int g = blockIdx.y;
  const int R = with_real ? 2 * bs : bs;
  const int64_t total = (int64_t)T * R * ld, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % ld);
  const int64_t tr = e / ld;
  const int r = (int)(tr % R), t = (int)(tr / R);
  const int b = *it_dev % nb;
  float v = 0.f;
  if (k < n) {
    const float* set = src[2 * g + (r < bs ? 0 : 1)];
    v = set[((int64_t)b * bs + (r % bs)) * T * n + (int64_t)t * n + k];
  }
  dst[g * dst_net + e] = v;
}

__global__ __launch_bounds__(256) void cls_cell_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ gh,
                                                           float* __restrict__ gates, float* __restrict__ h, int R, int t, int64_t gi_net,
                                                           int64_t h_net) {
  const int g = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= R * VUNET_CLS_H) return;
  const int r = e / VUNET_CLS_H, j = e - r * VUNET_CLS_H;
  const int64_t o = g * gi_net + ((int64_t)t * R + r) * VUNET_CLS_G + j;
  float* hp = h + g * h_net + (int64_t)t * R * VUNET_CLS_H;
  const float rg = sigmoid_f(gi[o] + gh[o]);
  const float zg = sigmoid_f(gi[o + VUNET_CLS_H] + gh[o + VUNET_CLS_H]);
  const float ng = tanhf(gi[o + 2 * VUNET_CLS_H] + rg * gh[o + 2 * VUNET_CLS_H]);
  const float hprev = hp[e];
  gates[o] = rg;
  gates[o + VUNET_CLS_H] = zg;
  gates[o + 2 * VUNET_CLS_H] = ng;
  hp[(int64_t)R * VUNET_CLS_H + e] = ng + zg * (hprev - ng);   // torch's form: h' = n + z (h - n)
}

// One workgroup per net.  Fixed-order reductions: each thread's rows in ascending order, then a tree over the 256 threads.
__global__ __launch_bounds__(256) void cls_head_kernel(const float* __restrict__ hT, int64_t h_net, const float* __restrict__ params,
                                                       int bs, int with_real, const int32_t* __restrict__ it_dev, int slot_off,
                                                       float* __restrict__ loss_out, float* __restrict__ acc_out, int ld_curve,
                                                       float* __restrict__ dh, float* __restrict__ grad, int64_t grad_net) {
  __shared__ float dl[2 * VUNET_CLS_MAX_BS];
  __shared__ float red[3][256];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int R = with_real ? 2 * bs : bs;
  const float* P = params + (int64_t)g * VUNET_CLS_P;
  const float* H = hT + g * h_net;
  const float* w = P + VUNET_CLS_OFF_FCW;
  const float fb = P[VUNET_CLS_OFF_FCB];
  float s_acc = 0.f, s_f = 0.f, s_r = 0.f;
  const float inv = 1.f / (float)bs;
  for (int r = tid; r < R; r += 256) {
    const float* hr = H + (int64_t)r * VUNET_CLS_H;
    float x = 0.f;
    for (int j = 0; j < VUNET_CLS_H; ++j) x = fmaf(w[j], hr[j], x);
    x += fb;
    const float sg = sigmoid_f(x);
    // BCEWithLogits: (1 - y) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|))
    const float ls = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));
    if (r < bs) {
      s_acc += sg;
      s_f += x - ls;
      dl[r] = sg * inv;
    } else {
      s_r -= ls;
      dl[r] = (sg - 1.f) * inv;
    }
  }
  red[0][tid] = s_acc;
  red[1][tid] = s_f;
  red[2][tid] = s_r;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + o];
    __syncthreads();
  }
  const int slot = *it_dev + slot_off;
  if (tid == 0) {
    acc_out[(int64_t)g * ld_curve + slot] = red[0][0] * inv;
    if (with_real) loss_out[(int64_t)g * ld_curve + slot] = red[1][0] * inv + red[2][0] * inv;
  }
  if (!dh) return;
  // dfc1.w[j] = sum_r dl[r] h_T[r][j] (thread j, rows ascending);  dfc1.b = sum_r dl[r];  dh_T[r][j] = dl[r] w[j]
  float* G = grad + g * grad_net;
  float* D = dh + (int64_t)g * R * VUNET_CLS_H;   // [nets][R][256]
  const int j = tid;
  float gw = 0.f, gb = 0.f;
  const float wj = w[j];
  for (int r = 0; r < R; ++r) {
    gw = fmaf(dl[r], H[(int64_t)r * VUNET_CLS_H + j], gw);
    gb += dl[r];
    D[(int64_t)r * VUNET_CLS_H + j] = dl[r] * wj;
  }
  G[VUNET_CLS_OFF_FCW + j] = gw;
  if (j == 0) G[VUNET_CLS_OFF_FCB] = gb;
}

__global__ __launch_bounds__(256) void cls_cell_bwd_kernel(float* __restrict__ gi, float* __restrict__ gh, const float* __restrict__ gates,
                                                           const float* __restrict__ h, const float* __restrict__ dh,
                                                           float* __restrict__ dh_prev, int R, int t, int64_t gi_net, int64_t h_net,
                                                           int64_t dh_net) {
  const int g = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= R * VUNET_CLS_H) return;
  const int r = e / VUNET_CLS_H, j = e - r * VUNET_CLS_H;
  const int64_t o = g * gi_net + ((int64_t)t * R + r) * VUNET_CLS_G + j;
  const float rg = gates[o], zg = gates[o + VUNET_CLS_H], ng = gates[o + 2 * VUNET_CLS_H];
  const float hn = gh[o + 2 * VUNET_CLS_H];
  const float hprev = h[g * h_net + (int64_t)t * R * VUNET_CLS_H + e];
  const float d = dh[g * dh_net + e];
  const float dn = d * (1.f - zg), dz = d * (hprev - ng);
  const float an = dn * (1.f - ng * ng);
  const float ar = an * hn * rg * (1.f - rg);
  const float az = dz * zg * (1.f - zg);
  gi[o] = ar;
  gi[o + VUNET_CLS_H] = az;
  gi[o + 2 * VUNET_CLS_H] = an;
  gh[o] = ar;
  gh[o + VUNET_CLS_H] = az;
  gh[o + 2 * VUNET_CLS_H] = an * rg;
  dh_prev[g * dh_net + e] = d * zg;
}

// a * b + c in two roundings, as torch's mul_ / add_ pair leaves it.  hipcc contracts a * b + c into one fma by default, and HIP's
// __fmul_rn / __fadd_rn are the plain operators, which it contracts just the same: the pragma is what pins the roundings.
__device__ __forceinline__ float mul_then_add(float a, float b, float c) {
#pragma clang fp contract(off)
  return a * b + c;
}

__global__ __launch_bounds__(256) void cls_sgd_kernel(float* __restrict__ params, const float* __restrict__ grad, float* __restrict__ buf,
                                                      int S, float lr, float momentum, const int32_t* __restrict__ it_dev) {
  const int g = blockIdx.y;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= VUNET_CLS_P) return;
  const float* G = grad + (int64_t)g * S * VUNET_CLS_P + e;
  float gv = G[0];
  if (e < VUNET_CLS_OFF_FCW)
    for (int s = 1; s < S; ++s) gv += G[(int64_t)s * VUNET_CLS_P];
  const int64_t o = (int64_t)g * VUNET_CLS_P + e;
  // torch.optim.SGD (dampening 0, no nesterov): buf = g first, then buf = momentum buf + g;  p = p + (-lr) buf
  const float b = *it_dev == 0 ? gv : mul_then_add(momentum, buf[o], gv);
  buf[o] = b;
  params[o] = mul_then_add(-lr, b, params[o]);
}

__global__ __launch_bounds__(256) void cls_reg_loss_kernel(const float* __restrict__ pred, int ldp, int64_t pred_net,
                                                           const float* __restrict__ xo, const float* __restrict__ xc, int T, int bs, int nb,
                                                           const int32_t* __restrict__ start_dev, const int32_t* __restrict__ it_dev,
                                                           int slot_off, float* __restrict__ loss_out, float* __restrict__ de_out,
                                                           int ld_curve, float* __restrict__ dpred) {
  __shared__ float red[2][256];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int st = start_dev[g], b = *it_dev % nb;
  const float* P = pred + g * pred_net;
  float* D = dpred + g * pred_net;
  const float inv = 1.f / (float)bs;
  float sl = 0.f, sd = 0.f;
  for (int r = tid; r < bs; r += 256) {
    const int64_t row = ((int64_t)b * bs + r) * T * VUNET_CLS_NIN + (int64_t)st * VUNET_CLS_NIN;
    const float* tg = xo + row;
    float q = 0.f;
    for (int k = 0; k < VUNET_CLS_NIN; ++k) {
      const float u = P[(int64_t)r * ldp + k] - tg[k];
      q = fmaf(u, u, q);
    }
    const float nr = sqrtf(q);
    sl += nr;
    const float sc = nr > 0.f ? inv / nr : 0.f;   // torch.norm's backward: x / ||x||, 0 at ||x|| = 0
    for (int k = 0; k < VUNET_CLS_NIN; ++k) D[(int64_t)r * ldp + k] = (P[(int64_t)r * ldp + k] - tg[k]) * sc;
    if (xc) {
      float q2 = 0.f;
      for (int k = 0; k < VUNET_CLS_NIN; ++k) {
        const float u = xc[row + k] - tg[k];
        q2 = fmaf(u, u, q2);
      }
      sd += sqrtf(q2);
    }
  }
  red[0][tid] = sl;
  red[1][tid] = sd;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[0][tid] += red[0][tid + o];
      red[1][tid] += red[1][tid + o];
    }
    __syncthreads();
  }
  if (tid) return;
  const int slot = *it_dev + slot_off;
  loss_out[(int64_t)g * ld_curve + slot] = red[0][0] * inv;
  if (xc) de_out[(int64_t)g * ld_curve + slot] = red[1][0] * inv;
}

__global__ __launch_bounds__(256) void cls_adam_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                       const float* __restrict__ g, int64_t n, vunet_seq_adam_hp hp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const int64_t o = blockIdx.y * n + e;
  const AdamResolved h = adam_resolve(hp);
  float pv = p[o], mv = m[o], vv = v[o];
  adam_update(h, g[o], pv, mv, vv);
  p[o] = pv;
  m[o] = mv;
  v[o] = vv;
}

__global__ void cls_tick_kernel(int32_t* it_dev, int64_t* step_dev) {
  if (it_dev) *it_dev = *it_dev + 1;
  if (step_dev) *step_dev = *step_dev + 1;
}

}  // namespace

extern "C" int vunet_seq_cls_gemm_run(const vunet_seq_cls_gemm* d, void* stream) {
  if (!d || !d->A || !d->B || !d->C || d->M < 1 || d->N < 1 || d->K < 1 || d->nets < 1 || d->nets > 65535 || d->split < 1 ||
      d->split > 64)
    return VUNET_ERR_ARG;
  const int64_t tiles = (int64_t)((d->M + 31) / 32) * ((d->N + 31) / 32);
  if (tiles > 0x7fffffff) return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_gemm_kernel, dim3((unsigned)tiles, d->nets, d->split), dim3(64), 0, (hipStream_t)stream, *d);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_gather(const float* const* src_dev, int32_t nets, int32_t T, int32_t n, int32_t ld, int32_t bs, int32_t nb,
                                    int32_t with_real, const int32_t* it_dev, float* dst, int64_t dst_net, void* stream) {
  if (!src_dev || !it_dev || !dst || nets < 1 || nets > 65535 || T < 1 || n < 1 || ld < n || bs < 1 || nb < 1) return VUNET_ERR_ARG;
  const int64_t total = (int64_t)T * (with_real ? 2 : 1) * bs * ld;
  if (dst_net < total) return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_gather_kernel, dim3((unsigned)((total + 255) / 256), nets), dim3(256), 0, (hipStream_t)stream, src_dev, T, n, ld, bs, nb,
               with_real, it_dev, dst, dst_net);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_cell_fwd(const float* gi, const float* gh, float* gates, float* h, int32_t nets, int32_t T, int32_t R, int32_t t,
                                      int64_t gi_net, int64_t h_net, void* stream) {
  if (!gi || !gh || !gates || !h || nets < 1 || nets > 65535 || R < 1 || t < 0 || t >= T) return VUNET_ERR_ARG;
  if (gi_net < (int64_t)T * R * VUNET_CLS_G || h_net < (int64_t)(T + 1) * R * VUNET_CLS_H) return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_cell_fwd_kernel, dim3(R, nets), dim3(256), 0, (hipStream_t)stream, gi, gh, gates, h, R, t, gi_net, h_net);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_head(const float* hT, int64_t h_net, const float* params, int32_t nets, int32_t bs, int32_t with_real,
                                  const int32_t* it_dev, int32_t slot_off, float* loss_out, float* acc_out, int32_t ld_curve, float* dh,
                                  float* grad, int64_t grad_net, void* stream) {
  if (!hT || !params || !it_dev || !acc_out || nets < 1 || bs < 1 || bs > VUNET_CLS_MAX_BS || ld_curve < 1) return VUNET_ERR_ARG;
  if ((with_real && !loss_out) || (dh && (!with_real || !grad)) || h_net < (int64_t)(with_real ? 2 : 1) * bs * VUNET_CLS_H)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_head_kernel, dim3(nets), dim3(256), 0, (hipStream_t)stream, hT, h_net, params, bs, with_real, it_dev, slot_off, loss_out,
               acc_out, ld_curve, dh, grad, grad_net);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_cell_bwd(float* gi, float* gh, const float* gates, const float* h, const float* dh, float* dh_prev, int32_t nets,
                                      int32_t T, int32_t R, int32_t t, int64_t gi_net, int64_t h_net, int64_t dh_net, void* stream) {
  if (!gi || !gh || !gates || !h || !dh || !dh_prev || nets < 1 || nets > 65535 || R < 1 || t < 0 || t >= T) return VUNET_ERR_ARG;
  if (gi_net < (int64_t)T * R * VUNET_CLS_G || h_net < (int64_t)(T + 1) * R * VUNET_CLS_H || dh_net < (int64_t)R * VUNET_CLS_H)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_cell_bwd_kernel, dim3(R, nets), dim3(256), 0, (hipStream_t)stream, gi, gh, gates, h, dh, dh_prev, R, t, gi_net, h_net,
               dh_net);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_sgd(float* params, const float* grad, float* buf, int32_t nets, int32_t S, float lr, float momentum,
                                 const int32_t* it_dev, void* stream) {
  if (!params || !grad || !buf || !it_dev || nets < 1 || nets > 65535 || S < 1) return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_sgd_kernel, dim3((VUNET_CLS_P + 255) / 256, nets), dim3(256), 0, (hipStream_t)stream, params, grad, buf, S, lr, momentum,
               it_dev);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_reg_loss(const float* pred, int32_t ldp, int64_t pred_net, const float* xo, const float* xc, int32_t T,
                                      int32_t bs, int32_t nb, const int32_t* start_dev, const int32_t* it_dev, int32_t slot_off,
                                      float* loss_out, float* de_out, int32_t ld_curve, float* dpred, int32_t nets, void* stream) {
  if (!pred || !xo || !start_dev || !it_dev || !loss_out || !dpred || (xc && !de_out) || ldp < VUNET_CLS_NIN || T < 1 || bs < 1 ||
      nb < 1 || nets < 1 || ld_curve < 1 || pred_net < (int64_t)bs * ldp)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_reg_loss_kernel, dim3(nets), dim3(256), 0, (hipStream_t)stream, pred, ldp, pred_net, xo, xc, T, bs, nb, start_dev, it_dev,
               slot_off, loss_out, de_out, ld_curve, dpred);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_adam(float* p, float* m, float* v, const float* g, int32_t nets, int64_t n, const vunet_seq_adam_hp* hp,
                                  void* stream) {
  if (!p || !m || !v || !g || !hp || nets < 1 || nets > 65535 || n < 1 || !hp->lr_dev || !hp->step_dev) return VUNET_ERR_ARG;
  if (hp->beta1 < 0.f || hp->beta1 >= 1.f || hp->beta2 < 0.f || hp->beta2 >= 1.f || hp->eps < 0.f) return VUNET_ERR_ARG;
  VUNET_LAUNCH(cls_adam_kernel, dim3((unsigned)((n + 255) / 256), nets), dim3(256), 0, (hipStream_t)stream, p, m, v, g, n, *hp);
  return vunet_check_launch();
}

extern "C" int vunet_seq_cls_tick(int32_t* it_dev, int64_t* step_dev, void* stream) {
  VUNET_LAUNCH(cls_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, it_dev, step_dev);
  return vunet_check_launch();
}
