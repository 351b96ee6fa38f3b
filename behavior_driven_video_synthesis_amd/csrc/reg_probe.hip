// The post-hoc pose-regressor probe of the image experiments' run_inference (experiments/shape_and_pose_net.py:921-995,
// experiments/vunet.py:745-805; models/vunets.py:786-824).  Interface: include/vunet_reg_probe.h.
//
// The regressor's linears, its input gradients and the weight-gradient sweep fused into Adam run on the seq family's kernels
// (vunet_seq_linear, vunet_seq_dx, vunet_seq_dz_finish, vunet_seq_dw).  What is here is the part those do not cover:
//   * reg_embed_kernel: an embedder is B <= 64 rows against a [128][8192] (or [128][2048]) matrix -- 8 row tiles of W, 0.5 MB
//     each.  Without a split that is 8 workgroups on 256 CUs, each waiting on its own weight stream.  K is cut into S slabs across
//     workgroups (grid M / 16 x S: 256 workgroups at the shipped sizes), each writes a RAW partial slab.
//   * reg_embed_finish_kernel: adds the slabs in slab order with bias and ReLU into the first linear layer's concat operand.  (Its
//     one consumer of the slabs reads every value once: the case in which csrc/seq.hip found a split to pay.)
//   * reg_loss_kernel: mean_b ||pred_b - tgt_b||_2, its gradient, and the append to the device-side loss course.
// Nothing uses float atomics; every sum has a fixed order.  Stores are plain (vector) stores.
#include "common.h"
#include "../../include/vunet_reg_probe.h"

namespace {

// grid (M / 16, S), 256 threads = 4 waves.  Lane l of a wave: i = l & 15 (weight row of the tile / batch row of a batch tile),
// kq = l >> 4.  In a K chunk of 16 the lane holds k = 4 kq .. 4 kq + 3 of its row: ONE 16-byte load of W and one of X per batch
// tile, the same k for the A (weights) and B (batch) operand of MFMA step j = 0 .. 3.  Wave w takes chunks w, w + 4, ... of the
// slab.  D: lane holds batch row l & 15 of its tile, output rows 4 (l >> 4) + r of the weight tile.
// LDS per workgroup: 4 waves x NB batch tiles x 64 lanes x 16 bytes = 4 KB (NB = 1) .. 16 KB (NB = 4).
template <int NB>
__global__ __launch_bounds__(256) void reg_embed_kernel(const float* __restrict__ x, const float* __restrict__ w, int M, int K, int L,
                                                        float* __restrict__ part) {
  __shared__ float4 red[4][NB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * 16, s = blockIdx.y;
  const int Bp = NB * 16;
  const size_t k_lo = (size_t)s * L;
  const float* __restrict__ wp = w + (size_t)(m0 + i) * K + k_lo + 4 * kq;
  const float* __restrict__ xp = x + (size_t)i * K + k_lo + 4 * kq;
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nit = L >> 6;   // L % 64 == 0: every wave has the same number of chunks
  for (int it0 = 0; it0 < nit; it0 += 4) {   // four chunks' loads in flight, then their matrix steps, k ascending
    float4 wv[4], xv[4][NB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = wave + 4 * (it0 + u < nit ? it0 + u : nit - 1);   // (a short tail re-reads the last chunk; not used)
      wv[u] = *reinterpret_cast<const float4*>(wp + 16 * c);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) xv[u][nb] = *reinterpret_cast<const float4*>(xp + (size_t)nb * 16 * K + 16 * c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (it0 + u >= nit) break;
      const float wa[4] = {wv[u].x, wv[u].y, wv[u].z, wv[u].w};
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const float xb[4] = {xv[u][nb].x, xv[u][nb].y, xv[u][nb].z, xv[u][nb].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j], xb[j], acc[nb], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) red[wave][nb][lane] = make_float4(acc[nb][0], acc[nb][1], acc[nb][2], acc[nb][3]);
  __syncthreads();
  for (int e = threadIdx.x; e < NB * 64; e += 256) {
    const int nb = e >> 6, l = e & 63;
    float4 v = red[0][nb][l];
    v = add4(v, red[1][nb][l]);
    v = add4(v, red[2][nb][l]);
    v = add4(v, red[3][nb][l]);
    const int b = nb * 16 + (l & 15), m = m0 + 4 * (l >> 4);
    *reinterpret_cast<float4*>(part + ((size_t)s * Bp + b) * M + m) = v;
  }
}

__global__ __launch_bounds__(256) void reg_embed_finish_kernel(const float* __restrict__ part, int S, const float* __restrict__ bias,
                                                               int B, int Bp, int M, float* __restrict__ y, int ldy, int col_off) {
  const int m4 = M >> 2;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= Bp * m4) return;
  const int b = e / m4, m = 4 * (e - b * m4);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (b < B) {
    const size_t per = (size_t)Bp * M, o = (size_t)b * M + m;
    v = *reinterpret_cast<const float4*>(part + o);
    for (int s = 1; s < S; ++s) v = add4(v, *reinterpret_cast<const float4*>(part + (size_t)s * per + o));
    v = add4(v, *reinterpret_cast<const float4*>(bias + m));
    v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
  }
  *reinterpret_cast<float4*>(y + (size_t)b * ldy + col_off + m) = v;
}

// one workgroup of four waves; wave w takes rows w, w + 4, ...: the row's norm, then its gradient.  The mean adds the rows in
// row order.
__global__ __launch_bounds__(256) void reg_loss_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ tgt, int ldt,
                                                       int B, int Bp, int n, float* __restrict__ dpred, float* __restrict__ last,
                                                       float* __restrict__ losses, int cap, int* __restrict__ cursor) {
  __shared__ float norms[64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float inv_b = 1.f / (float)B;
  for (int b = wave; b < Bp; b += 4) {
    float ss = 0.f;
    if (b < B)
      for (int d = lane; d < n; d += 64) {
        const float r = pred[(size_t)b * ldp + d] - tgt[(size_t)b * ldt + d];
        ss += r * r;
      }
    const float nrm = sqrtf(wave_sum(ss));
    const float sc = nrm > 0.f ? inv_b / nrm : 0.f;
    for (int d = lane; d < ldp; d += 64) {
      float g = 0.f;
      if (b < B && d < n) g = (pred[(size_t)b * ldp + d] - tgt[(size_t)b * ldt + d]) * sc;
      dpred[(size_t)b * ldp + d] = g;
    }
    if (lane == 0 && b < B) norms[b] = nrm;
  }
  __syncthreads();
  if (threadIdx.x) return;
  float sum = 0.f;
  for (int b = 0; b < B; ++b) sum += norms[b];
  const float L = sum * inv_b;
  last[0] = L;
  if (losses) {
    const int i = *cursor;
    if (i >= 0 && i < cap) losses[i] = L;
    *cursor = i + 1;
  }
}

}  // namespace

extern "C" int vunet_reg_probe_embed(const float* x, const float* w, int32_t B, int32_t M, int32_t K, int32_t S, float* part,
                                     void* stream) {
  if (!x || !w || !part || B < 1 || B > 64 || M < 16 || M % 16 || K < 64 || S < 1 || S > 65535) return VUNET_ERR_ARG;
  if ((int64_t)K % (64 * (int64_t)S)) return VUNET_ERR_ARG;
  const int L = K / S;
  const dim3 grid(M / 16, S);
  hipStream_t st = (hipStream_t)stream;
  switch ((B + 15) / 16) {
    case 1: VUNET_LAUNCH(reg_embed_kernel<1>, grid, dim3(256), 0, st, x, w, M, K, L, part); break;
    case 2: VUNET_LAUNCH(reg_embed_kernel<2>, grid, dim3(256), 0, st, x, w, M, K, L, part); break;
    case 3: VUNET_LAUNCH(reg_embed_kernel<3>, grid, dim3(256), 0, st, x, w, M, K, L, part); break;
    case 4: VUNET_LAUNCH(reg_embed_kernel<4>, grid, dim3(256), 0, st, x, w, M, K, L, part); break;
    default: return VUNET_ERR_ARG;
  }
  return vunet_check_launch();
}

extern "C" int vunet_reg_probe_embed_finish(const float* part, int32_t S, const float* bias, int32_t B, int32_t M, float* y, int32_t ldy,
                                            int32_t col_off, void* stream) {
  if (!part || !bias || !y || S < 1 || B < 1 || B > 64 || M < 16 || M % 16 || ldy % 4 || col_off < 0 || col_off % 4 || col_off + M > ldy)
    return VUNET_ERR_ARG;
  const int Bp = (B + 15) / 16 * 16;
  const int n4 = Bp * (M / 4);
  VUNET_LAUNCH(reg_embed_finish_kernel, dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, part, S, bias, B, Bp, M, y, ldy,
               col_off);
  return vunet_check_launch();
}

extern "C" int vunet_reg_probe_loss(const float* pred, int32_t ldp, const float* tgt, int32_t ldt, int32_t B, int32_t n, float* dpred,
                                    float* last, float* losses, int32_t cap, int32_t* cursor, void* stream) {
  if (!pred || !tgt || !dpred || !last || B < 1 || B > 64 || n < 1 || ldp < n || ldt < n) return VUNET_ERR_ARG;
  if (losses && (!cursor || cap < 0)) return VUNET_ERR_ARG;
  const int Bp = (B + 15) / 16 * 16;
  VUNET_LAUNCH(reg_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pred, ldp, tgt, ldt, B, Bp, n, dpred, last, losses, cap,
               cursor);
  return vunet_check_launch();
}
