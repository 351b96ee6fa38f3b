// "p2": 3x3 / pad 1 / stride 1 convolution (forward and data gradient) on PRE-SPLIT activations -- the h2 arithmetic of
// conv_h2_kernel.h (two scaled fp16 terms per fp32 operand, three partial products, fp32 accumulation on the fp16 matrix
// cores) with the operand conversion done ONCE, by the producer of a tensor, instead of by every workgroup that stages it.
//
// Why.  conv_h2_kernel converts its input tile while staging it: loads to registers, scale, split, ds_write -- per element
// ~8 vector instructions, repeated by each of the M / 64 workgroups that read the tile and 1.25x by the halo: for VGG19
// conv4_x (512 -> 512 channels) every activation is converted TEN times per layer, and every workgroup first reduces 4 KB
// of partial |x| maxima to find the scale.  Here a tensor lives in HBM as two fp16 planes (hi, lo) in channel blocks of 8
// -- 16-byte units that ARE the B fragment of v_mfma_f32_16x16x32_f16 -- written by the producing kernel's epilogue
// (values are in its registers anyway), with a one-pixel zero border, so that the consumer's staging is a linear
// LDS-DMA copy (global_load_lds_dwordx4): no registers, no VALU, no ds_write, no bounds logic.  HBM bytes per element
// are the same as fp32 (2 + 2).
//
// Layout of a planes tensor ("P2"), logical shape [N][C][H][W], C % 8 == 0:
//     fp16  [2 planes][N][C / 8][H + 2][W + 2][8]        plane 0 = hi, plane 1 = lo;  s x = hi + lo / 2^11,  s = 2^e
//     int32 meta[128]:  [0] e (scale exponent)   [16 .. 79] 64 slots holding max |x| (fp32 bit patterns, atomicMax;
//                       zeroed by the caller before the producer runs): an UPPER BOUND of the largest stored magnitude
// The border rows / columns hold zeros and are never written by a producer: the caller zero-fills a buffer once and
// reuses it (ops.py keeps the VGG19 pass's buffers in a persistent arena).
//
// The scale of an OUTPUT cannot come from its maximum (unknown until the kernel has finished), so it comes from a bound:
//     |y| <= max_row( sum |w| ) * max|x| + max|shift|        (x's maximum IS known: its producer published it)
// rounded up to a power of two.  The bound is typically 2^5 .. 2^8 above the true maximum.  That costs nothing: the pair
// (hi, lo) represents s x with absolute error <= max(2^-23 |s x|, 2^-36) -- hi = f16(s x) has 11 bits, the remainder is
// scaled by 2^11 before it is rounded, and where hi goes subnormal the remainder still resolves 2^-36 -- so relative to the
// tensor's maximum the error stays at 2^-23 as long as that maximum sits above 2^-13 after scaling, i.e. for bounds up to
// 2^27 too large (tests/test_hip_p2.py: fp64 reference, inputs whose scale exponent is forced 2^20 too small).
//
// Work decomposition (NW waves; 16x16x32 MFMA: A = weights [16 rows][32 k], B = activations [32 k][16 pixels], the k of an
// instruction = 32 channels of ONE tap -- chunks of 32 input channels):
//   tile      16 NW output channels x (8 rows x CT columns) of one image; wave w: channel group w >> 2 (64 channels = 4
//             m-tiles), rows 2 (w & 3), 2 (w & 3) + 1 (2 CT / 16 pixel tiles): 4 x 4 accumulator tiles of 4 registers,
//             two sets (leading term / cross terms) = 128 VGPRs
//   xL        [XBUF][2 planes][4 k-quarters][10 x (CT + 2)] units, filled by LDS-DMA one chunk ahead (XBUF = 2: eight waves,
//             one workgroup per CU; also four waves with ONE term on small grids, see p2_route) or between chunks (XBUF = 1:
//             four waves, two workgroups per CU cover each other)
//   wL        [2][16 NW / 16 m-tiles][2 planes][64] the weight slab of ONE tap, by LDS-DMA one tap ahead; one barrier per tap
//   epilogue  combine, de-scale, + shift, ReLU (forward) -- scale by the OUTPUT's 2^e, split, pack; two lane rows exchange
//             halves (v_permlane16_swap) so that a lane holds the 8 channels of one 16-byte unit; data gradient: the unit is
//             masked by [forward activation != 0] read as two 16-byte units of the forward planes (the ReLU backward of the
//             layer below); max |y| published into the output's meta
#include <stdio.h>

#include <type_traits>

#include "common.h"
#include "split_h2.h"

namespace {

constexpr int P2_META = 128, P2_AMAX0 = 16, P2_NSLOT = 64;

struct P2Args {
  const uint4* x;        // input planes
  const int* xmeta;
  const uint4* w;        // weight image (vunet_p2_pack_weights)
  const float* wk;       // [0] max row sum of |w|, [1] max |shift|, [2] weight scale exponent (as a float)
  const float* shift;    // [M] or null
  const uint4* mask;     // planes shaped like y (data gradient: the forward activation of the layer below) or null
  uint4* y;
  int* ymeta;
  int N, C, H, W, M;
  int relu;
};

__device__ __forceinline__ void p2_dma(uint32_t voff, const void* sbase, uint32_t lds_addr) {
  // 64 lanes x 16 bytes from sbase + voff (per lane) to 1 KiB of LDS at the wave-uniform byte address lds_addr.  Inline
  // assembly for the reason given at h2_dma16 (conv_h2_kernel.h); retired by p2_dma_wait<N>() before the publishing barrier.
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(sbase), "s"(lds_addr)
               : "memory");
}
template <int N>
__device__ __forceinline__ void p2_dma_wait() {   // all but the N youngest transfers of this wave have landed
  static_assert(N == 0 || N == 1 || N == 2 || N == 4, "counts in use");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
}
__device__ __forceinline__ const void* p2_uniform_ptr(const void* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const void*)(((uint64_t)hi << 32) | lo);
}

union P2Unit {
  uint4 u;
  h2_f16x8 b;
};

// upper bound of the stored magnitudes of a planes tensor: the 64 slots of its meta, one per lane
__device__ __forceinline__ float p2_meta_amax(const int* meta, int lane) {
  return wave_max(__int_as_float(meta[P2_AMAX0 + (lane & (P2_NSLOT - 1))]));
}

// two lanes of adjacent lane rows (lane, lane ^ 16) exchange halves: see the epilogue
__device__ __forceinline__ void p2_swap16(uint32_t& a, uint32_t& b) {
  const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
  a = r[0];
  b = r[1];
}

// per 16-bit half: 0xFFFF where the half of t is non-zero (sign bits already cleared), else 0
__device__ __forceinline__ uint32_t p2_nonzero_halves(uint32_t t) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  u16x2 v = __builtin_bit_cast(u16x2, t);
  const u16x2 one = {1, 1}, all = {0xFFFF, 0xFFFF};
  v = __builtin_elementwise_min(v, one) * all;
  return __builtin_bit_cast(uint32_t, v);
}

// conv_p2_kernel / conv_p2a_kernel, once per term count (two terms: the arithmetic described above; one term: the hi planes only,
// one product per tap -- VUNET_TUNE_P2_TERMS).  Why textual inclusion and not a template parameter: see the header.
#define P2_TERMS 2
#include "conv_p2_kernel.h"
#undef P2_TERMS
#define P2_TERMS 1
#include "conv_p2_kernel.h"
#undef P2_TERMS

template <int CT, int TERMS>
int p2a_launch(const P2Args& a, hipStream_t st) {
  constexpr int XU = 4 * TERMS * 10 * (CT + 2), XS = (XU + 63) / 64 * 64, WU = 128 * 4 * TERMS;
  constexpr size_t lds = (size_t)(2 * XS + 2 * WU) * 16;
  const int blocks = a.N * (a.H / 8) * (a.W / CT) * (a.M / 128);
  void (*kern)(const P2Args);
  if constexpr (TERMS == 2) kern = conv_p2a_kernel<CT>;
  else kern = conv_p2a_kernel<CT, 1>;
  if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return VUNET_ERR_LAUNCH;
  VUNET_LAUNCH(kern, dim3((unsigned)blocks), dim3(512), lds, st, a);
  return vunet_check_launch();
}

template <int NW, int CT, int XBUF, int TERMS>
int p2_launch(const P2Args& a, hipStream_t st) {
  constexpr int XU = 4 * TERMS * 10 * (CT + 2), XS = (XU + 63) / 64 * 64, WU = 16 * NW * 4 * TERMS;
  constexpr size_t lds = (size_t)(XBUF * XS + 2 * WU) * 16;
  const int blocks = a.N * (a.H / 8) * (a.W / CT) * (a.M / (16 * NW));
  void (*kern)(const P2Args);
  if constexpr (TERMS == 2) kern = conv_p2_kernel<NW, CT, XBUF>;
  else kern = conv_p2_kernel<NW, CT, XBUF, 1>;
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return VUNET_ERR_LAUNCH;
  VUNET_LAUNCH(kern, dim3((unsigned)blocks), dim3(64 * NW), lds, st, a);
  return vunet_check_launch();
}

}  // namespace

static bool p2_shape_ok(const vunet_p2_desc* d) {
  if (!d || d->N < 1 || d->C < 32 || d->C % 32 || d->M < 64 || d->M % 64 || d->H < 8 || d->H % 8) return false;
  if (!(d->W == 16 || (d->W >= 32 && d->W % 32 == 0))) return false;
  // 32-bit byte offsets inside one image's planes (the lo plane sits a whole plane behind the hi plane)
  const double plane_bytes = (double)d->N * (d->C / 8) * (d->H + 2) * (d->W + 2) * 16.0;
  return plane_bytes * 2.0 < 4.0e9;
}

extern "C" int vunet_p2_conv_supported(const vunet_p2_desc* d) { return p2_shape_ok(d) ? 1 : 0; }

// waves per workgroup: eight / 128 channels (x double-buffered, one workgroup per CU) where that still fills the chip;
// otherwise four / 64 channels (two workgroups per CU, x single-buffered).  VUNET_TUNE_P2_FORM: 1 = four, 2 = eight (tests, A/B)
static int p2_form(const vunet_p2_desc* d) {
  const long px_tiles = (long)d->N * (d->H / 8) * (d->W / (d->W == 16 ? 16 : 32));
  const int force = g_vunet_tune[VUNET_TUNE_P2_FORM];
  const bool wide = d->M % 128 == 0 && (force == 2 || force == 3 || (force != 1 && px_tiles * (d->M / 128) >= 256));
  return wide ? 8 : 4;
}

// Which kernel runs a problem: the ONE decision behind vunet_p2_conv and vunet_p2_conv_variant.
// VUNET_TUNE_P2_TERMS: 0 / 2 = two terms per operand, three products per tap; 1 = one product per tap on the hi planes ("f16"
// mode), every launch, on the form the two-term rule picks; 3 = one product per tap for DATA-GRADIENT launches only
// ("f16grad" mode): a forward launch takes exactly the path of 0, a data gradient the four-wave one-term kernel -- measured
// faster than the eight-wave antiphase one on every VGG19 shape where the two-term rule picks eight waves
// (profiles/p2_f16grad_time.txt) -- unless VUNET_TUNE_P2_FORM = 2 / 3 asks for the antiphase one.  A one-term x tile is half
// the size, so the four-wave kernel can hold two of them and fetch the next chunk's tile one chunk ahead (XBUF = 2, 52 KiB,
// still two workgroups per CU) instead of between chunks: that wins where the launch has at most one workgroup per CU, so
// that no second resident workgroup covers the refill (conv4_1, conv5_x at batch 16: x1.08), and loses x0.93 - x0.97 on the
// large grids (same file).  VUNET_TUNE_P2_FORM = 1 keeps the single buffer (A/B, tests).
struct P2Route {
  int terms;       // 2 | 1
  int form;        // waves per workgroup: 4 | 8
  bool lockstep;   // two terms, eight waves: conv_p2_kernel<8, CT, 2> instead of the antiphase kernel (VUNET_TUNE_P2_FORM = 3)
  int xbuf;        // x tiles in LDS of conv_p2_kernel: four waves 1 (one term in "f16grad" mode: 1 | 2), eight waves 2
};
static P2Route p2_route(const vunet_p2_desc* d, bool dgrad) {
  const int mode = g_vunet_tune[VUNET_TUNE_P2_TERMS], force = g_vunet_tune[VUNET_TUNE_P2_FORM];
  if (mode == 3 && dgrad) {
    if (d->M % 128 == 0 && (force == 2 || force == 3)) return {1, 8, false, 2};
    const long wgs = (long)d->N * (d->H / 8) * (d->W / (d->W == 16 ? 16 : 32)) * (d->M / 64);
    return {1, 4, false, force != 1 && wgs <= 256 ? 2 : 1};
  }
  const int terms = mode == 1 ? 1 : 2, form = p2_form(d);
  // one term: no lockstep eight-wave variant (VUNET_TUNE_P2_FORM = 3 runs the antiphase kernel)
  return {terms, form, terms == 2 && force == 3, form == 8 ? 2 : 1};
}

extern "C" int vunet_p2_conv(const vunet_p2_desc* d, const void* x, const int32_t* xmeta, const void* w_image, const float* wk,
                             const float* shift, const void* mask, void* y, int32_t* ymeta, void* stream) {
  if (!d || !x || !xmeta || !w_image || !wk || !y || !ymeta) return VUNET_ERR_ARG;
  if (!p2_shape_ok(d)) return VUNET_ERR_UNSUPPORTED;
  if (((uintptr_t)x | (uintptr_t)w_image | (uintptr_t)y | (uintptr_t)mask | (uintptr_t)shift) & 15) return VUNET_ERR_ARG;
  P2Args a;
  a.x = (const uint4*)x; a.xmeta = xmeta; a.w = (const uint4*)w_image; a.wk = wk; a.shift = shift; a.mask = (const uint4*)mask;
  a.y = (uint4*)y; a.ymeta = ymeta;
  a.N = d->N; a.C = d->C; a.H = d->H; a.W = d->W; a.M = d->M; a.relu = d->relu;
  hipStream_t st = (hipStream_t)stream;
  // a data-gradient launch: no ReLU and no shift (a data gradient has neither; the descriptor does not say which image w is)
  const P2Route r = p2_route(d, d->relu == 0 && shift == nullptr);
  if (r.terms == 2) {
    if (d->W == 16) return r.form == 8 ? (r.lockstep ? p2_launch<8, 16, 2, 2>(a, st) : p2a_launch<16, 2>(a, st)) : p2_launch<4, 16, 1, 2>(a, st);
    return r.form == 8 ? (r.lockstep ? p2_launch<8, 32, 2, 2>(a, st) : p2a_launch<32, 2>(a, st)) : p2_launch<4, 32, 1, 2>(a, st);
  }
  if (r.form == 8 || r.xbuf == 1) {
    if (d->W == 16) return r.form == 8 ? p2a_launch<16, 1>(a, st) : p2_launch<4, 16, 1, 1>(a, st);
    return r.form == 8 ? p2a_launch<32, 1>(a, st) : p2_launch<4, 32, 1, 1>(a, st);
  }
  // (named last: the compiler emits kernels in the order of their first use, and a kernel's local labels carry its index)
  return d->W == 16 ? p2_launch<4, 16, 2, 1>(a, st) : p2_launch<4, 32, 2, 1>(a, st);
}

// the kernel instantiation vunet_p2_conv launches for this problem, in rocprofv3's spelling (bench.py's roofline keys).  The
// descriptor is all it has: relu == 0 stands for the data gradient
extern "C" int vunet_p2_conv_variant(const vunet_p2_desc* d, char* name, int32_t len) {
  if (!d || !name || len < 32) return VUNET_ERR_ARG;
  if (!p2_shape_ok(d)) return VUNET_ERR_UNSUPPORTED;
  const P2Route r = p2_route(d, d->relu == 0);
  const int ct = d->W == 16 ? 16 : 32;
  if (r.terms == 1) {
    if (r.form == 8) snprintf(name, (size_t)len, "conv_p2a_kernel<%d, 1>", ct);
    else snprintf(name, (size_t)len, "conv_p2_kernel<4, %d, %d, 1>", ct, r.xbuf);
    return VUNET_OK;
  }
  if (r.form == 8 && !r.lockstep) snprintf(name, (size_t)len, "conv_p2a_kernel<%d>", ct);
  else snprintf(name, (size_t)len, "conv_p2_kernel<%d, %d, %d>", r.form, ct, r.xbuf);
  return VUNET_OK;
}

// ------------------------------------------------------------------------------------------------ weight image
// w [Cout][Cin][3][3] fp32 (the layer's effective weights) -> image [K / 32 chunks][9 taps][R / 16 m-tiles][2 planes][4
// k-quarters][16 rows] 16-byte units of 8 fp16 (k = 32 chunk + 8 quarter + j), scaled by 2^ew so that max |w| lands in
// [2^13, 2^14), split as the activations are.  forward: rows R = Cout, k = Cin, tap (kh, kw).  data gradient: rows = Cin,
// k = Cout, tap (kh', kw') holds w[..][2 - kh'][2 - kw'] (the mirrored tap: the kernel itself is the same).
// wk: [0] max over rows of sum |w| over (k, taps), [1] max |shift| (forward; 0 for the data gradient), [2] ew.
namespace {
__global__ __launch_bounds__(256) void p2_wstat_kernel(const float* __restrict__ w, int Cout, int Cin, int dgrad,
                                                       float* __restrict__ rows) {
  // one workgroup per row of the image's matrix: rows[2 r] = sum |w|, rows[2 r + 1] = max |w|
  __shared__ float red[8];
  const int r = blockIdx.x;
  float s = 0.f, m = 0.f;
  const int K = dgrad ? Cout : Cin;
  for (int i = threadIdx.x; i < K * 9; i += 256) {
    const int k = i / 9, t = i - 9 * k;
    const float v = fabsf(dgrad ? w[((size_t)k * Cin + r) * 9 + t] : w[((size_t)r * Cin + k) * 9 + t]);
    s += v;
    m = fmaxf(m, v);
  }
  s = wave_sum(s);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s;
    red[4 + (threadIdx.x >> 6)] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rows[2 * r] = (red[0] + red[1]) + (red[2] + red[3]);
    rows[2 * r + 1] = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
  }
}
__global__ __launch_bounds__(256) void p2_wk_kernel(const float* __restrict__ rows, int R, const float* __restrict__ shift,
                                                    int nshift, float* __restrict__ wk) {
  __shared__ float red[12];
  float s = 0.f, m = 0.f, b = 0.f;
  for (int i = threadIdx.x; i < R; i += 256) {
    s = fmaxf(s, rows[2 * i]);
    m = fmaxf(m, rows[2 * i + 1]);
  }
  for (int i = threadIdx.x; i < nshift; i += 256) b = fmaxf(b, fabsf(shift[i]));
  s = wave_max(s);
  m = wave_max(m);
  b = wave_max(b);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s;
    red[4 + (threadIdx.x >> 6)] = m;
    red[8 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
    // (the bound is used as  wk[0] * max|x| + wk[1]  in fp32: a relative 2^-20 covers the roundings of the sums)
    wk[0] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3])) * (1.f + 1e-6f);
    wk[1] = fmaxf(fmaxf(red[8], red[9]), fmaxf(red[10], red[11]));
    wk[2] = (float)h2_scale_exp(mx);
    wk[3] = mx;
  }
}
__global__ __launch_bounds__(256) void p2_wpack_kernel(const float* __restrict__ w, int Cout, int Cin, int dgrad,
                                                       const float* __restrict__ wk, uint4* __restrict__ img) {
  const int R = dgrad ? Cin : Cout, K = dgrad ? Cout : Cin;
  const int MT = R / 16;
  const size_t units = (size_t)(K / 32) * 9 * MT * 2 * 64;
  const float sw = h2_pow2((int)wk[2]);
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (size_t)gridDim.x * 256) {
    size_t v = u;
    const int l = (int)(v & 63);
    v >>= 6;
    const int p = (int)(v & 1);
    v >>= 1;
    const int mt = (int)(v % MT);
    v /= MT;
    const int tap = (int)(v % 9);
    const int ch = (int)(v / 9);
    const int row = mt * 16 + (l & 15), k0 = ch * 32 + (l >> 4) * 8;
    const int kh = tap / 3, kw = tap - 3 * kh;
    float e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + j;
      const float x = dgrad ? w[(((size_t)k * Cin + row) * 3 + (2 - kh)) * 3 + (2 - kw)] : w[(((size_t)row * Cin + k) * 3 + kh) * 3 + kw];
      e[j] = x * sw;
    }
    uint32_t h[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) h2_split2(e[2 * j], e[2 * j + 1], h[j], lo[j]);
    img[u] = p ? make_uint4(lo[0], lo[1], lo[2], lo[3]) : make_uint4(h[0], h[1], h[2], h[3]);
  }
}
}  // namespace

extern "C" int vunet_p2_weight_image_bytes(int32_t Cout, int32_t Cin, int32_t dgrad) {
  const int R = dgrad ? Cin : Cout, K = dgrad ? Cout : Cin;
  if (R < 16 || R % 16 || K < 32 || K % 32 || (int64_t)R * K > (1 << 22)) return 0;
  return (K / 32) * 9 * (R / 16) * 2 * 64 * 16;
}

extern "C" int vunet_p2_pack_weights(const float* w, const float* shift, int32_t Cout, int32_t Cin, int32_t dgrad, void* image,
                                     float* wk, float* workspace, void* stream) {
  if (!w || !image || !wk || !workspace) return VUNET_ERR_ARG;
  if (vunet_p2_weight_image_bytes(Cout, Cin, dgrad) == 0) return VUNET_ERR_UNSUPPORTED;
  const int R = dgrad ? Cin : Cout;
  hipStream_t st = (hipStream_t)stream;
  VUNET_LAUNCH(p2_wstat_kernel, dim3((unsigned)R), dim3(256), 0, st, w, (int)Cout, (int)Cin, (int)dgrad, workspace);
  VUNET_LAUNCH(p2_wk_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, R, dgrad ? nullptr : shift,
               (dgrad || !shift) ? 0 : (int)Cout, wk);
  const size_t units = (size_t)vunet_p2_weight_image_bytes(Cout, Cin, dgrad) / 16;
  size_t nb = (units + 255) / 256;
  if (nb > 2048) nb = 2048;
  VUNET_LAUNCH(p2_wpack_kernel, dim3((unsigned)nb), dim3(256), 0, st, w, (int)Cout, (int)Cin, (int)dgrad, (const float*)wk,
               (uint4*)image);
  return vunet_check_launch();
}

// wk alone (no image): the bound constants of a layer the p2 kernels do not run themselves (the 3-channel first layer,
// csrc/conv_thin.hip: vunet_p2_conv_first).  w [Cout][Cin][3][3]; workspace: 2 * Cout floats.
extern "C" int vunet_p2_weight_bound(const float* w, const float* shift, int32_t Cout, int32_t Cin, float* wk, float* workspace,
                                     void* stream) {
  if (!w || !wk || !workspace || Cout < 1 || Cin < 1) return VUNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  VUNET_LAUNCH(p2_wstat_kernel, dim3((unsigned)Cout), dim3(256), 0, st, w, (int)Cout, (int)Cin, 0, workspace);
  VUNET_LAUNCH(p2_wk_kernel, dim3(1), dim3(256), 0, st, (const float*)workspace, (int)Cout, shift, shift ? (int)Cout : 0, wk);
  return vunet_check_launch();
}

// ------------------------------------------------------------------------------------------------ converters
namespace {
// fp32 NCHW -> planes.  amax: partial |x| maxima (n_amax floats, e.g. the 512 of vunet_absmax_partials / a producer's tag):
// the scale comes from the true maximum.  One thread per unit: 8 channels of one pixel (coalesced across lanes in x).
__global__ __launch_bounds__(256) void p2_from_nchw_kernel(const float* __restrict__ x, const float* __restrict__ amax, int n_amax,
                                                           int relu, uint4* __restrict__ y, int* __restrict__ ymeta, int N, int C,
                                                           int H, int W) {
  __shared__ float red[4];
  float m = 0.f;
  for (int i = threadIdx.x; i < n_amax; i += 256) m = fmaxf(m, amax[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  const int e = h2_scale_exp(m);
  const float s = h2_pow2(e);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ymeta[0] = e;
    ymeta[P2_AMAX0] = __float_as_int(m);
  }
  const int CB = C >> 3, Hp = H + 2, Wp = W + 2;
  const size_t HW = (size_t)H * W, total = (size_t)N * CB * HW, plane = (size_t)N * CB * Hp * Wp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int xw = (int)(i % W);
    size_t t = i / W;
    const int yh = (int)(t % H);
    t /= H;   // = n * CB + cb
    const float* src = x + (t * 8) * HW + (size_t)yh * W + xw;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = src[j * HW];
      if (relu) f = f > 0.f ? f : 0.f;
      v[j] = f * s;
    }
    uint4 h, l;
    h2_split2(v[0], v[1], h.x, l.x);
    h2_split2(v[2], v[3], h.y, l.y);
    h2_split2(v[4], v[5], h.z, l.z);
    h2_split2(v[6], v[7], h.w, l.w);
    const size_t o = (t * Hp + (yh + 1)) * Wp + (xw + 1);
    y[o] = h;
    y[plane + o] = l;
  }
}
__device__ __forceinline__ void p2_unpack(const uint4& h, const uint4& l, float inv, float* v) {
  const uint32_t hs[4] = {h.x, h.y, h.z, h.w}, ls[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const h2_f16x2 a = __builtin_bit_cast(h2_f16x2, hs[j]), b = __builtin_bit_cast(h2_f16x2, ls[j]);
    v[2 * j] = ((float)a[0] + (float)b[0] * (1.f / 2048.f)) * inv;
    v[2 * j + 1] = ((float)a[1] + (float)b[1] * (1.f / 2048.f)) * inv;
  }
}
__global__ __launch_bounds__(256) void p2_to_nchw_kernel(const uint4* __restrict__ x, const int* __restrict__ xmeta,
                                                         float* __restrict__ y, int N, int C, int H, int W) {
  const int CB = C >> 3, Hp = H + 2, Wp = W + 2;
  const float inv = h2_pow2(-xmeta[0]);
  const size_t HW = (size_t)H * W, total = (size_t)N * CB * HW, plane = (size_t)N * CB * Hp * Wp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int xw = (int)(i % W);
    size_t t = i / W;
    const int yh = (int)(t % H);
    t /= H;
    const size_t o = (t * Hp + (yh + 1)) * Wp + (xw + 1);
    float v[8];
    p2_unpack(x[o], x[plane + o], inv, v);
    float* dst = y + (t * 8) * HW + (size_t)yh * W + xw;
#pragma unroll
    for (int j = 0; j < 8; ++j) dst[j * HW] = v[j];
  }
}
}  // namespace

extern "C" int vunet_p2_from_nchw(const float* x, const float* amax, int32_t n_amax, int32_t relu, void* y, int32_t* ymeta,
                                  int32_t N, int32_t C, int32_t H, int32_t W, void* stream) {
  if (!x || !amax || n_amax < 1 || !y || !ymeta || C % 8 || N < 1) return VUNET_ERR_ARG;
  const size_t total = (size_t)N * (C / 8) * H * W;
  size_t nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  VUNET_LAUNCH(p2_from_nchw_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, amax, (int)n_amax, (int)relu, (uint4*)y,
               (int*)ymeta, (int)N, (int)C, (int)H, (int)W);
  return vunet_check_launch();
}

extern "C" int vunet_p2_to_nchw(const void* x, const int32_t* xmeta, float* y, int32_t N, int32_t C, int32_t H, int32_t W,
                                void* stream) {
  if (!x || !xmeta || !y || C % 8 || N < 1) return VUNET_ERR_ARG;
  const size_t total = (size_t)N * (C / 8) * H * W;
  size_t nb = (total + 255) / 256;
  if (nb > 4096) nb = 4096;
  VUNET_LAUNCH(p2_to_nchw_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, (const uint4*)x, (const int*)xmeta, y, (int)N,
               (int)C, (int)H, (int)W);
  return vunet_check_launch();
}
