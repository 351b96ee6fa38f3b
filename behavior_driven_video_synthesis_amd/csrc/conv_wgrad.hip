// Weight-gradient of the fused convolution on fp32 MFMA (generic geometry).
//
//   dW[co][tap][ci] = sum_px dy[co][px] * f(x)[ci][px (+) tap]        (K = pixels)
//
// A workgroup owns a (WM*32 output channels) x (all taps x 32 input channels) block of dW and a
// contiguous range of 32-pixel chunks (split-K over pixels).  Per chunk it stages
//   dyL[co][33]      -- the dy rows of its output channels (coalesced along pixels)
//   fxL[tap][ci][33] -- the im2col'ed, prologue-activated input (ELU / dropout applied here)
// into LDS (row pitch 33 dwords: conflict-free transposed reads), then every wave runs
// v_mfma_f32_32x32x2_f32 with A = dy (lane: co, k-half: pixel parity) and B = f(x) (lane: ci).
// Partial results go to per-split slabs (deterministic; summed by vunet_weightnorm_bwd).
// The per-channel sum of dy (gradient of the folded shift) falls out of the A fragments.
#include "common.h"
#include "conv_wgrad_route.h"

struct WgradArgs {
  vunet_wgrad_desc d;
  const float* x1;
  const float* x2;
  const float* dy;
  float* slabs;
  float* dshift;
  int NP, HoWo, HsWs, T, Ctot, Coutp, nchunks, cps;
  InAct in1, in2;
};

template <int WM, int WN, int NTW>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradArgs a_in) {
  WgradArgs a = a_in;
  inact_resolve(a.in1);
  inact_resolve(a.in2);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int MB = 32 * WM;
  constexpr int PITCH = 33;
  float* dyL = smem;                 // [MB][33]
  float* fxL = smem + MB * PITCH;    // [T*32][33]

  const vunet_wgrad_desc& d = a.d;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int wm = wave / WN, wn = wave % WN;
  const int q = tid & 31, rgrp = tid >> 5;

  const int split = blockIdx.x;
  const int ci0 = blockIdx.y * 32;
  const int co0 = blockIdx.z * MB;
  const int T = a.T;

  f32x16 acc[NTW];
#pragma unroll
  for (int i = 0; i < NTW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float dsum = 0.f;

  const int c_begin = split * a.cps;
  const int c_end = min(c_begin + a.cps, a.nchunks);

  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    // ---- this thread's pixel
    const int P = chunk * 32 + q;
    const bool pv = P < a.NP;
    const int Pc = pv ? P : 0;
    const int n = Pc / a.HoWo;
    const int rem = Pc - n * a.HoWo;
    const int oh = rem / d.Wo, ow = rem - oh * d.Wo;
    const int ih0 = oh * d.stride - d.pad, iw0 = ow * d.stride - d.pad;

    __syncthreads();  // previous chunk's MFMA reads are done
    // ---- stage dy rows
#pragma unroll 4
    for (int i = 0; i < MB / 8; ++i) {
      const int col = rgrp + 8 * i, co = co0 + col;
      const bool ok = pv && co < d.Cout;
      const float v = a.dy[ok ? (size_t)(n * d.Cout + co) * a.HoWo + rem : 0];
      dyL[col * PITCH + q] = ok ? v : 0.f;
    }
    // ---- stage im2col'ed activated input rows
    int kh = 0, kw = 0;
    for (int tap = 0; tap < T; ++tap) {
      const int ih = ih0 + kh, iw = iw0 + kw;
      const bool tv = pv && (unsigned)ih < (unsigned)d.Hs && (unsigned)iw < (unsigned)d.Ws;
      const int sp = ih * d.Ws + iw;
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int cl = rgrp + 8 * ii, ci = ci0 + cl;
        const bool ok = tv && ci < a.Ctot;
        const bool first = ci < d.C1;
        const int off = first ? (n * d.C1 + ci) * a.HsWs + sp : (n * d.C2 + (ci - d.C1)) * a.HsWs + sp;
        const float* __restrict__ xs = (first || !a.x2) ? a.x1 : a.x2;
        const float raw = xs[ok ? off : 0];  // unconditional load
        const float v = apply_in_act(first ? a.in1 : a.in2, raw, (uint32_t)off);
        fxL[(tap * 32 + cl) * PITCH + q] = ok ? v : 0.f;
      }
      if (++kw == d.KW) { kw = 0; ++kh; }
    }
    __syncthreads();

    // ---- MFMA over the 32 pixels of the chunk (16 k-steps of 2)
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
      const float av = dyL[(wm * 32 + j) * PITCH + 2 * ks + h];
      dsum += av;
#pragma unroll
      for (int i = 0; i < NTW; ++i) {
        const int nt = wn + WN * i;
        if (nt < T) {
          const float bv = fxL[(nt * 32 + j) * PITCH + 2 * ks + h];
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[i], 0, 0, 0);
        }
      }
    }
  }

  // ---- write the partial slab  [split][Coutp][T*Ctot]
  const size_t KT = (size_t)T * a.Ctot;
  float* slab = a.slabs + (size_t)split * a.Coutp * KT;
  const int ci = ci0 + j;
#pragma unroll
  for (int i = 0; i < NTW; ++i) {
    const int nt = wn + WN * i;
    if (nt >= T || ci >= a.Ctot) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co < d.Cout) slab[(size_t)co * KT + (size_t)nt * a.Ctot + ci] = acc[i][r];
    }
  }
  if (wn == 0 && blockIdx.y == 0) {
    const float tot = dsum + __shfl_xor(dsum, 32, 64);
    const int co = co0 + wm * 32 + j;
    if (h == 0 && co < a.Coutp) a.dshift[(size_t)split * a.Coutp + co] = co < d.Cout ? tot : 0.f;
  }
}

// ---- the plan: the first family that takes the problem fills it; everything below reads it
static WgradRoute wgrad_route(const vunet_wgrad_desc* d) {
  WgradRoute r = {};
  if (vunet_wgrad_x6_plan(d, &r) || vunet_wgrad_direct_plan(d, &r) || vunet_wgrad_thin_plan(d, &r) || vunet_wgrad_tiled_plan(d, &r))
    return r;
  r.family = WGRAD_GENERIC;
  const int T = d->KH * d->KW;
  r.WM = d->Cout > 64 ? 4 : (d->Cout > 32 ? 2 : 1);
  if (T > 9 && r.WM == 4) r.WM = 2;
  r.WN = 4 / r.WM;
  r.NTW = T == 1 ? 1 : (T <= 9 ? (r.WM == 4 ? 9 : (r.WM == 2 ? 5 : 3)) : (r.WM == 2 ? 8 : 4));
  r.ntiles = (int)(((int64_t)d->N * d->Ho * d->Wo + 31) / 32);   // 32-pixel chunks
  r.ciblocks = (d->C1 + d->C2 + 31) / 32, r.coblocks = (d->Cout + 32 * r.WM - 1) / (32 * r.WM);
  int S = 768 / (r.ciblocks * r.coblocks);
  if (S > r.ntiles) S = r.ntiles;  // small maps: one 32-pixel chunk per workgroup rather than a serial chunk loop
  // (capping S to bound the slab volume was measured slower: the serial chunk loop costs more than the reduce)
  if (S < 1) S = 1;
  r.nslabs = S > 256 ? 256 : S;
  return r;
}

// character for character what the profiler keys and the tests hold
int wgrad_route_name(const WgradRoute& r, char* name, int len) {
  switch (r.family) {
    case WGRAD_X6: return snprintf(name, len, "conv_wgrad_x6_kernel<%d>", r.MTW);
    case WGRAD_H2: return snprintf(name, len, "conv_wgrad_h2_kernel<%d>", r.MTW);
    case WGRAD_DIRECT:
      if (r.s2_ncot) return snprintf(name, len, "conv_wgrad_s2_kernel");   // (bare: the same for its three instantiations)
      return snprintf(name, len, "conv_wgrad_direct_kernel<%d, %s, %d>", r.S, r.W4 ? "true" : "false", r.T);
    case WGRAD_THIN: return snprintf(name, len, "conv_wgrad_thin_kernel");
    case WGRAD_TILED: return snprintf(name, len, "conv_wgrad_tiled_kernel<%d, %d, %d, %d>", r.MTW, r.TH, r.KS, r.ST);
    default: return snprintf(name, len, "conv_wgrad_kernel<%d, %d, %d>", r.WM, r.WN, r.NTW);
  }
}

// layers whose weight gradient runs on the direct kernel and is a short launch: batched (vunet_conv2d_wgrad_multi)
static bool wgrad_route_batchable(const WgradRoute& r, const vunet_wgrad_desc* d) {
  // (A/B: VUNET_WGRAD_BATCH_PIX moves the bound between "latency" and "work"; read once per process)
  static const int64_t bound = [] { const char* e = getenv("VUNET_WGRAD_BATCH_PIX"); return e ? atoll(e) : WGRAD_BATCH_PIX; }();
  return r.family == WGRAD_DIRECT && (int64_t)d->N * d->Ho * d->Wo <= bound;
}

extern "C" int vunet_conv2d_wgrad_batchable(const vunet_wgrad_desc* d) {
  return d && wgrad_route_batchable(wgrad_route(d), d) ? 1 : 0;
}

extern "C" int vunet_conv2d_wgrad_multi(const vunet_wgrad_item* items, int32_t n, void* stream) {
  if (n < 0 || (n > 0 && !items)) return VUNET_ERR_ARG;
  constexpr int MAXN = 256;
  if (n > MAXN) return VUNET_ERR_ARG;
  WgradRoute routes[MAXN];
  int form[MAXN], idx[MAXN];
  for (int i = 0; i < n; ++i) {
    routes[i] = wgrad_route(&items[i].d);
    if (!wgrad_route_batchable(routes[i], &items[i].d) || items[i].d.nsplit < 1) return VUNET_ERR_UNSUPPORTED;
    form[i] = routes[i].form;
  }
  for (int i = 0; i < n; ++i) {
    if (form[i] < 0) continue;           // already launched with an earlier item of its form
    int cnt = 0;
    const int f = form[i];
    for (int k = i; k < n; ++k)
      if (form[k] == f) { idx[cnt++] = k; form[k] = -1; }
    const int rc = vunet_wgrad_direct_launch_multi(items, routes, idx, cnt, (hipStream_t)stream);
    if (rc != VUNET_OK) return rc;
  }
  return VUNET_OK;
}

extern "C" int vunet_conv2d_wgrad_wants_split(const vunet_wgrad_desc* d) {
  return d && wgrad_route_wants_split(wgrad_route(d)) ? 1 : 0;
}

extern "C" int vunet_conv2d_wgrad_variant(const vunet_wgrad_desc* d, char* name, int32_t len) {
  if (!d || !name || len < 8) return VUNET_ERR_ARG;
  wgrad_route_name(wgrad_route(d), name, len);
  return VUNET_OK;
}

extern "C" int vunet_conv2d_wgrad_nsplit(const vunet_wgrad_desc* d) { return d ? wgrad_route(d).nslabs : VUNET_ERR_ARG; }

template <int WM, int WN, int NTW>
static int launch_wgrad(const WgradRoute& r, const WgradArgs& wa, hipStream_t st) {
  dim3 grid(wa.d.nsplit, r.ciblocks, r.coblocks), block(256);
  const size_t lds = (size_t)(32 * WM + wa.T * 32) * 33 * sizeof(float);
  if (lds > 64 * 1024)
    hipFuncSetAttribute((const void*)conv_wgrad_kernel<WM, WN, NTW>, hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)lds);
  VUNET_LAUNCH((conv_wgrad_kernel<WM, WN, NTW>), grid, block, lds, st, wa);
  return vunet_check_launch();
}

static int wgrad_generic_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st) {
  const vunet_wgrad_desc* d = &it.d;
  WgradArgs wa;
  wgrad_fill(wa, it);
  wa.T = d->KH * d->KW;
  wa.NP = d->N * d->Ho * d->Wo;
  wa.nchunks = r.ntiles;
  wa.HoWo = d->Ho * d->Wo;
  wa.HsWs = d->Hs * d->Ws;
  wa.cps = (wa.nchunks + d->nsplit - 1) / d->nsplit;
  if (wa.T > 16) return VUNET_ERR_UNSUPPORTED;
  switch (r.WM * 16 + r.NTW) {   // <WM, WN = 4 / WM, NTW> as wgrad_route picked them
    case 4 * 16 + 1: return launch_wgrad<4, 1, 1>(r, wa, st);
    case 2 * 16 + 1: return launch_wgrad<2, 2, 1>(r, wa, st);
    case 1 * 16 + 1: return launch_wgrad<1, 4, 1>(r, wa, st);
    case 4 * 16 + 9: return launch_wgrad<4, 1, 9>(r, wa, st);
    case 2 * 16 + 5: return launch_wgrad<2, 2, 5>(r, wa, st);
    case 1 * 16 + 3: return launch_wgrad<1, 4, 3>(r, wa, st);
    case 2 * 16 + 8: return launch_wgrad<2, 2, 8>(r, wa, st);
    default: return launch_wgrad<1, 4, 4>(r, wa, st);
  }
}

extern "C" int vunet_conv2d_wgrad_a2(const vunet_wgrad_desc* d, const float* x1, const float* x2, const float* dy,
                                     float* slabs, float* dshift, const float* amax_x, const float* amax_x2,
                                     const float* amax_dy, void* stream) {
  if (!d || !x1 || !dy || !slabs || !dshift) return VUNET_ERR_ARG;
  if (d->C2 > 0 && !x2) return VUNET_ERR_ARG;
  if (d->nsplit < 1 || d->KH < 1 || d->KW < 1) return VUNET_ERR_ARG;
  const int64_t in_elems = (int64_t)d->N * (d->C1 > d->C2 ? d->C1 : d->C2) * d->Hs * d->Ws;
  const int64_t out_elems = (int64_t)d->N * d->Cout * d->Ho * d->Wo;
  if (in_elems >= (1ll << 31) || out_elems >= (1ll << 31)) return VUNET_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const WgradRoute r = wgrad_route(d);
  if ((r.family == WGRAD_H2 || r.family == WGRAD_DIRECT) && (!amax_x || !amax_dy)) return VUNET_ERR_ARG;
  const vunet_wgrad_item it = {*d, x1, x2, dy, slabs, dshift, amax_x, amax_x2, amax_dy};
  switch (r.family) {
    case WGRAD_X6: return vunet_wgrad_x6_launch(r, it, st);
    case WGRAD_H2: return vunet_wgrad_h2_launch(r, it, st);
    case WGRAD_DIRECT: return vunet_wgrad_direct_launch(r, it, st);
    case WGRAD_THIN: return vunet_wgrad_thin_launch(r, it, st);
    case WGRAD_TILED: return vunet_wgrad_tiled_launch(r, it, st);
    default: return wgrad_generic_launch(r, it, st);
  }
}

extern "C" int vunet_conv2d_wgrad(const vunet_wgrad_desc* d, const float* x1, const float* x2, const float* dy,
                                  float* slabs, float* dshift, const float* amax_x, const float* amax_dy, void* stream) {
  return vunet_conv2d_wgrad_a2(d, x1, x2, dy, slabs, dshift, amax_x, nullptr, amax_dy, stream);
}
