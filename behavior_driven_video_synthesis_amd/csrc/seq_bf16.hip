// Half-size weights for flow INFERENCE (include/vunet_seq_bf16.h): the MLP layers of csrc/seq.hip with the weight matrices stored
// as bf16 tile images and multiplied on v_mfma_f32_16x16x32_bf16.
//
// A sample pass of the flow streams every weight once (csrc/seq.hip: 2.5 GB of fp32 at the reference size) and its fp32-input
// MFMA runs at 1/16 of the bf16 rate, so the pass sits near both limits; the remaining lever is bytes.  Here a [16 rows][32 k]
// chunk of W is 1 KB (one 16-byte load per lane, already in the A-operand order) and the activations keep fp32 information: each
// operand value is split in registers into three bf16 terms that sum to it exactly, three MFMA per chunk into one fp32
// accumulator, smallest term first.  The result is the fp32-accurate product with the bf16-rounded weights -- the split-term idea
// of csrc/conv_bf16.hip turned onto the operand.
//
// Geometry, K split over the waves, the LDS reduction in wave order, the split head's raw slabs and the epilogue (bias, LeakyReLU /
// Tanh, row or tile output) are those of seq_linear_kernel; the operand is read as that kernel reads it (rows or xt tiles): lane l
// of a wave holds batch row l & 15 and k = 8 (l >> 4) .. + 7 of a chunk there, which IS the B-operand map of the bf16 instruction.
#include "common.h"
#include "../../include/vunet_seq_bf16.h"
#include "seq_linear_args.h"

namespace {

typedef __bf16 seq_bf16x8 __attribute__((ext_vector_type(8)));

union SeqFrag {
  uint4 u;
  seq_bf16x8 b;
};

using SeqLinear16Args = SeqLinearBaseArgs<uint16_t>;   // w: bf16 tile images [M / 16][K / 32][64][8]

// x == t0 + t1 + t2: the upper 16 bits of the running remainder, three times (both subtractions are exact).  Values a, b are
// elements 2 p, 2 p + 1 of the fragments: bf16 element j sits in bits 16 (j & 1) of word j / 2.
__device__ __forceinline__ void seq16_split_pair(float a, float b, unsigned& t0, unsigned& t1, unsigned& t2) {
  const unsigned a0 = __float_as_uint(a) & 0xffff0000u, b0 = __float_as_uint(b) & 0xffff0000u;
  t0 = (a0 >> 16) | b0;
  const float ra = a - __uint_as_float(a0), rb = b - __uint_as_float(b0);
  const unsigned a1 = __float_as_uint(ra) & 0xffff0000u, b1 = __float_as_uint(rb) & 0xffff0000u;
  t1 = (a1 >> 16) | b1;
  const float sa = ra - __uint_as_float(a1), sb = rb - __uint_as_float(b1);
  t2 = (__float_as_uint(sa) >> 16) | (__float_as_uint(sb) & 0xffff0000u);
}

template <int NB, int U>
struct Seq16GroupRegs {
  uint4 wv[U];
  float4 xv[NB][U][2];
};

// the loads of a group of U chunks (c0, c0 + WAVES, ...): one weight tile (read once per pass by this one workgroup: streamed
// past the caches' retention), the operand of NB batch tiles
template <int NB, int U, int WAVES, int LAY>
__device__ __forceinline__ void seq16_group_load(const SeqLinear16Args& a, const uint16_t* __restrict__ w, const float* __restrict__ x,
                                                 int c0, Seq16GroupRegs<NB, U>& r) {
#pragma unroll
  for (int u = 0; u < U; ++u) r.wv[u] = nt_load4(w + 512 * (size_t)(c0 + WAVES * u));
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (LAY & 2) {
        const float* xp = x + (size_t)nb * 16 * a.K + 512 * (c0 + WAVES * u);
        r.xv[nb][u][0] = *reinterpret_cast<const float4*>(xp);
        r.xv[nb][u][1] = *reinterpret_cast<const float4*>(xp + 256);
      } else {
        const float* xp = x + (size_t)nb * 16 * a.ldx + 32 * (c0 + WAVES * u);
        r.xv[nb][u][0] = *reinterpret_cast<const float4*>(xp);
        r.xv[nb][u][1] = *reinterpret_cast<const float4*>(xp + 4);
      }
    }
}

// ... and its matrix steps: chunk by chunk, batch tile by batch tile; per chunk t2, t1, t0 (include/vunet_seq_bf16.h)
template <int NB, int U>
__device__ __forceinline__ void seq16_group_mfma(const Seq16GroupRegs<NB, U>& r, f32x4 (&acc)[NB]) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    SeqFrag wa;
    wa.u = r.wv[u];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const float4 lo = r.xv[nb][u][0], hi = r.xv[nb][u][1];
      SeqFrag t0, t1, t2;
      seq16_split_pair(lo.x, lo.y, t0.u.x, t1.u.x, t2.u.x);
      seq16_split_pair(lo.z, lo.w, t0.u.y, t1.u.y, t2.u.y);
      seq16_split_pair(hi.x, hi.y, t0.u.z, t1.u.z, t2.u.z);
      seq16_split_pair(hi.z, hi.w, t0.u.w, t1.u.w, t2.u.w);
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa.b, t2.b, acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa.b, t1.b, acc[nb], 0, 0, 0);
      acc[nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa.b, t0.b, acc[nb], 0, 0, 0);
    }
  }
}

template <int NB, int U, int WAVES, int LAY>
__device__ __forceinline__ void seq16_linear_group(const SeqLinear16Args& a, const uint16_t* __restrict__ w, const float* __restrict__ x,
                                                   int c0, f32x4 (&acc)[NB]) {
  Seq16GroupRegs<NB, U> r;
  seq16_group_load<NB, U, WAVES, LAY>(a, w, x, c0, r);
  __builtin_amdgcn_sched_barrier(0);   // all loads of the group in flight before the first use (csrc/seq.hip)
  seq16_group_mfma<NB, U>(r, acc);
}

// grid (M / 16, S, nets), 64 WAVES threads.  Lane l: i = l & 15 (weight row / batch row), kq = l >> 4.  D: lane holds batch row
// i of its tile, output rows 4 kq + r of the weight tile (the C/D map does not depend on the input type).
// LAY: bit 1 -- the operand is xt tiles, bit 2 -- the output is the next layer's xt tiles (the weights are always images).
template <int NB, int WAVES, int LAY>
__global__ __launch_bounds__(64 * WAVES) void seq_linear_bf16w_kernel(SeqLinear16Args a) {
  __shared__ float4 red[WAVES][NB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * 16, net = blockIdx.z;
  const int kb = a.K / a.S, nchunk = kb >> 5;
  // tile m0 / 16 of the image starts at bf16 index m0 K; the chunks of this workgroup's K range at + (y kb / 32) 512
  const uint16_t* __restrict__ w = a.w[net] + (size_t)m0 * a.K + (size_t)blockIdx.y * kb * 16 + 8 * lane;
  const float* __restrict__ x = (LAY & 2) ? a.x + (a.shared_in ? 0 : (size_t)net * a.Bp * a.K) + (size_t)blockIdx.y * kb * 16 + 4 * lane
                                          : a.x + (a.shared_in ? 0 : (size_t)net * a.Bp * a.ldx) + (size_t)i * a.ldx +
                                                (size_t)blockIdx.y * kb + 8 * kq;
  f32x4 acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this wave's chunks: wave, wave + WAVES, ... (ascending k), in groups of UMAX, then 2, then 1
  // (16 waves share the CU's registers: 128 each)
  constexpr int UMAX = WAVES == 16 ? (NB == 1 ? 4 : 2) : (NB <= 2 ? 4 : 2);
  int c = wave;
  for (; c + WAVES * (UMAX - 1) < nchunk; c += WAVES * UMAX) seq16_linear_group<NB, UMAX, WAVES, LAY>(a, w, x, c, acc);
  if constexpr (UMAX == 4)
    if (c + WAVES < nchunk) {
      seq16_linear_group<NB, 2, WAVES, LAY>(a, w, x, c, acc);
      c += 2 * WAVES;
    }
  for (; c < nchunk; c += WAVES) seq16_linear_group<NB, 1, WAVES, LAY>(a, w, x, c, acc);
  // every wave's partial -> LDS; wave w < NB adds them in wave order for batch tile w and finishes that tile
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) red[wave][nb][lane] = make_float4(acc[nb][0], acc[nb][1], acc[nb][2], acc[nb][3]);
  __syncthreads();
  if (wave >= NB) return;
  const int nb = wave;
  float4 v = red[0][nb][lane];
#pragma unroll 3
  for (int q = 1; q < WAVES; ++q) v = add4(v, red[q][nb][lane]);
  const size_t col = (size_t)m0 + 4 * kq;   // row n = 16 nb + i
  if (a.S > 1) {   // a raw partial slab: seq_coupling_kernel adds the slabs in slab order, the bias and the tanh
    float* ys = a.y + ((size_t)net * a.S + blockIdx.y) * a.Bp * a.M + col;
    *reinterpret_cast<float4*>(ys + (size_t)(nb * 16 + i) * a.M) = v;
    return;
  }
  const float* bias = a.bias[net];
  const int act = a.act[net];
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias) bv = *reinterpret_cast<const float4*>(bias + col);
  float4 t = add4(v, bv);
  t = make_float4(seq_act(t.x, act), seq_act(t.y, act), seq_act(t.z, act), seq_act(t.w, act));
  if constexpr (LAY & 4) {
    // the next layer's operand tile: columns m0 + 4 kq .. + 3 of batch row i are chunk m0 / 32, slot 2 (m0 / 16 & 1) + kq / 2,
    // half kq & 1 there (include/vunet_seq_tiled.h)
    float* yt = a.y + (size_t)net * a.Bp * a.M + ((size_t)(nb * (a.M >> 5) + (m0 >> 5)) * 2 + (kq & 1)) * 256 +
                (i + 16 * (2 * ((m0 >> 4) & 1) + (kq >> 1))) * 4;
    *reinterpret_cast<float4*>(yt) = t;
  } else {
    *reinterpret_cast<float4*>(a.y + (size_t)net * a.Bp * a.M + col + (size_t)(nb * 16 + i) * a.M) = t;
  }
}

// round-to-nearest-even on the bit pattern; every NaN -> 0x7FC0 (what torch's float -> bfloat16 cast gives)
__device__ __forceinline__ unsigned seq16_bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// wt16[mt][c][l][j] = bf16(w[16 mt + (l & 15)][32 c + 8 (l >> 4) + j]): one thread per lane slot (8 values, 16 bytes) of the image
__global__ __launch_bounds__(256) void seq_pack_tiles_bf16_kernel(const float* __restrict__ w, int ld, int M, int K,
                                                                  uint16_t* __restrict__ wt16) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)M * K / 8) return;
  const int l = (int)(idx & 63);
  const size_t tc = idx >> 6;   // mt * (K / 32) + c
  const int nck = K >> 5, mt = (int)(tc / nck), c = (int)(tc - (size_t)mt * nck);
  const float* src = w + (size_t)(16 * mt + (l & 15)) * ld + 32 * c + 8 * (l >> 4);
  const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
  uint4 o;
  o.x = seq16_bf16_rne(lo.x) | (seq16_bf16_rne(lo.y) << 16);
  o.y = seq16_bf16_rne(lo.z) | (seq16_bf16_rne(lo.w) << 16);
  o.z = seq16_bf16_rne(hi.x) | (seq16_bf16_rne(hi.y) << 16);
  o.w = seq16_bf16_rne(hi.z) | (seq16_bf16_rne(hi.w) << 16);
  reinterpret_cast<uint4*>(wt16)[idx] = o;
}

}  // namespace

extern "C" int vunet_seq_pack_tiles_bf16(const float* w, int32_t ld, int32_t M, int32_t K, uint16_t* wt16, void* stream) {
  if (!w || !wt16 || M < 16 || M % 16 || K < 32 || K % 32 || ld < K || ld % 4) return VUNET_ERR_ARG;
  const size_t n8 = (size_t)M * K / 8;
  VUNET_LAUNCH(seq_pack_tiles_bf16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, ld, M, K, wt16);
  return vunet_check_launch();
}

extern "C" int vunet_seq_linear_bf16w(const vunet_seq_linear_desc* d, int32_t layout, const uint16_t* w0, const uint16_t* w1,
                                      const float* x, const float* bias0, const float* bias1, float* y, void* stream) {
  if (!d || !w0 || !x || !y) return VUNET_ERR_ARG;
  if (layout < 0 || layout > 7 || !(layout & VUNET_SEQ_TILED_W)) return VUNET_ERR_UNSUPPORTED;   // 1 / 3 / 5 / 7
  if (!seq_linear_desc_ok(d, layout, w1)) return VUNET_ERR_ARG;
  SeqLinear16Args a{};
  seq_linear_fill(a, d, w0, w1, x, bias0, bias1, y);
  const dim3 grid(d->M / 16, d->S, d->nets);
  hipStream_t st = (hipStream_t)stream;
  const auto launch = [&](auto nb, auto waves, auto lay) {
    VUNET_LAUNCH((seq_linear_bf16w_kernel<nb(), waves(), lay()>), grid, dim3(64 * waves()), 0, st, a);
  };
  if (!seq_dispatch<0, 2, 4, 6>(a.Bp / 16, seq_linear_wide(d->K / d->S, d->B), layout & 6, launch)) return VUNET_ERR_ARG;
  return vunet_check_launch();
}
