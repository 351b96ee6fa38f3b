// Nearest training-set neighbours of generated behaviour (lib/figures.py:258-262 in code space, :268-277 in pose space).
// Interface, arithmetic and limits: include/vunet_seq_nn.h.
//
// The reference scans the whole training set on the host once per query.  Here one launch streams the bank once per tile of
// queries: workgroup (chunk, tile) holds the tile in LDS, each of its four waves takes rows chunk start + wave, + 4, ... and
// keeps, in lane qi, the best (distance, index) of query qi over its rows.  A row's sum is a per-lane partial in a fixed element
// order followed by a fixed butterfly, so it depends on the row's values alone.  The waves' bests are folded per workgroup into
// one candidate per (chunk, query); a second small kernel folds the candidates per query.  Every fold applies nn_better, a
// total order (NaN first, then the distance, then the index): no atomics, and the result does not depend on the fold's shape.
#include "common.h"
#include "../../include/vunet_seq_nn.h"

namespace {

constexpr int NN_THREADS = 256;
constexpr int NN_WAVES = NN_THREADS / 64;
constexpr int QT_C = VUNET_NN_QT_CODES;
constexpr int QT_P = VUNET_NN_QT_POSES;
constexpr int NN_KMAX = VUNET_NN_MAX_H / 256;   // float4 per lane and row: a wave covers 256 floats per step

// numpy's argmin as an order on (distance, index): does a rank before b?
__device__ __forceinline__ bool nn_better(double ad, int ai, double bd, int bi) {
  const bool an = ad != ad, bn = bd != bd;
  if (an || bn) return an && (!bn || ai < bi);
  return ad < bd || (ad == bd && ai < bi);
}

__device__ __forceinline__ double nn_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);   // butterfly: every lane ends with the same value
  return v;
}

__device__ __forceinline__ double nn_inf() { return __longlong_as_double(0x7ff0000000000000LL); }

// the waves' bests (lane qi of every wave) -> one candidate per query of the tile, at [query][chunk]
template <int QT>
__device__ __forceinline__ void nn_store_candidates(double bd, int bi, double* wd, int* wi, int tile, int Q, int64_t chunk,
                                                    int64_t chunks, double* __restrict__ cand_d, int* __restrict__ cand_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane < QT) {
    wd[wave * QT + lane] = bd;
    wi[wave * QT + lane] = bi;
  }
  __syncthreads();
  if (threadIdx.x < QT) {
    double d = wd[threadIdx.x];
    int i = wi[threadIdx.x];
#pragma unroll
    for (int w = 1; w < NN_WAVES; ++w) {
      const double od = wd[w * QT + threadIdx.x];
      const int oi = wi[w * QT + threadIdx.x];
      if (nn_better(od, oi, d, i)) {
        d = od;
        i = oi;
      }
    }
    const int64_t qg = (int64_t)tile * QT + threadIdx.x;
    if (qg < Q) {
      cand_d[qg * chunks + chunk] = d;
      cand_i[qg * chunks + chunk] = i;
    }
  }
}

// one row's 4 (lane + 64 k) .. + 3 elements, zeros past H (a zero in the row and in the query adds +0 to the sum)
template <bool VEC>
__device__ __forceinline__ void nn_load_row(const float* __restrict__ row, int H, int nk, int lane, float4 (&v)[NN_KMAX]) {
#pragma unroll
  for (int k = 0; k < NN_KMAX; ++k) {
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k < nk) {
      const int e = 4 * (lane + 64 * k);
      if constexpr (VEC) {
        if (e < H) v[k] = *reinterpret_cast<const float4*>(row + e);   // H % 4 == 0: e < H covers e + 3
      } else {
        if (e < H) v[k].x = row[e];
        if (e + 1 < H) v[k].y = row[e + 1];
        if (e + 2 < H) v[k].z = row[e + 2];
        if (e + 3 < H) v[k].w = row[e + 3];
      }
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(NN_THREADS) void nn_codes_kernel(const float* __restrict__ bank, int64_t ld, int N, const float* __restrict__ q,
                                                              int Q, int H, int64_t chunks, double* __restrict__ cand_d,
                                                              int* __restrict__ cand_i) {
  extern __shared__ __align__(16) unsigned char nn_smem[];
  const int nk = (H + 255) >> 8, Hp = nk << 8;
  float* qs = reinterpret_cast<float*>(nn_smem);                      // [QT_C][Hp], zeros past H and past Q
  double* wd = reinterpret_cast<double*>(qs + QT_C * Hp);             // [NN_WAVES][QT_C]
  int* wi = reinterpret_cast<int*>(wd + NN_WAVES * QT_C);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = blockIdx.x;
  const int tile = blockIdx.y;
  for (int idx = threadIdx.x; idx < QT_C * Hp; idx += NN_THREADS) {
    const int qi = idx / Hp, e = idx - qi * Hp;
    const int64_t qg = (int64_t)tile * QT_C + qi;
    qs[idx] = (qg < Q && e < H) ? q[qg * H + e] : 0.f;
  }
  __syncthreads();

  const int64_t r0 = chunk * VUNET_NN_CHUNK;
  const int64_t rend = r0 + VUNET_NN_CHUNK < (int64_t)N ? r0 + VUNET_NN_CHUNK : (int64_t)N;
  double bd = nn_inf();
  int bi = 0x7fffffff;
  float4 cur[NN_KMAX], nxt[NN_KMAX];
  int64_t r = r0 + wave;
  if (r < rend) nn_load_row<VEC>(bank + r * ld, H, nk, lane, cur);
  for (; r < rend; r += NN_WAVES) {
    const bool more = r + NN_WAVES < rend;
    if (more) nn_load_row<VEC>(bank + (r + NN_WAVES) * ld, H, nk, lane, nxt);   // in flight while this row is summed
    double acc[QT_C];
#pragma unroll
    for (int qi = 0; qi < QT_C; ++qi) acc[qi] = 0.0;
#pragma unroll
    for (int k = 0; k < NN_KMAX; ++k) {
      if (k < nk) {
        const float4 b = cur[k];
        const float* qk = qs + 4 * (lane + 64 * k);
#pragma unroll
        for (int qi = 0; qi < QT_C; ++qi) {
          const float4 a = *reinterpret_cast<const float4*>(qk + qi * Hp);
          const double d0 = (double)(b.x - a.x), d1 = (double)(b.y - a.y), d2 = (double)(b.z - a.z), d3 = (double)(b.w - a.w);
          // the square of an fp32 value is exact in float64: fma rounds once, as the product then the sum would
          acc[qi] = fma(d3, d3, fma(d2, d2, fma(d1, d1, fma(d0, d0, acc[qi]))));
        }
      }
    }
#pragma unroll
    for (int qi = 0; qi < QT_C; ++qi) {
      const double d = sqrt(nn_wave_sum(acc[qi]));
      if (lane == qi && nn_better(d, (int)r, bd, bi)) {
        bd = d;
        bi = (int)r;
      }
    }
    if (more) {
#pragma unroll
      for (int k = 0; k < NN_KMAX; ++k) cur[k] = nxt[k];
    }
  }
  nn_store_candidates<QT_C>(bd, bi, wd, wi, tile, Q, chunk, chunks, cand_d, cand_i);
}

// unNormalizeData (data/data_conversions_3d.py:178-211) of one used dimension, with numpy's promotion: float32 statistics keep
// x * std + mean in float32, float64 ones in float64.  Two roundings, as numpy does: no fused multiply-add.
__device__ __forceinline__ double nn_unnormalise(float v, double sd, double m, int f32) {
#pragma clang fp contract(off)
  if (f32) return (double)(v * (float)sd + (float)m);
  return (double)v * sd + m;
}

__global__ __launch_bounds__(NN_THREADS) void nn_poses_kernel(const float* __restrict__ bank, int N, const float* __restrict__ q, int Q,
                                                              int T, int J, int root, const double* __restrict__ mean,
                                                              const double* __restrict__ stdv, int f32, int64_t chunks,
                                                              double* __restrict__ cand_d, int* __restrict__ cand_i) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char nn_smem[];
  const int TJ = T * J, n = 3 * J;
  double* cq = reinterpret_cast<double*>(nn_smem);                    // [QT_P][3][TJ]: un-normalised, root-centred, by coordinate
  double* wd = cq + (size_t)QT_P * 3 * TJ;                            // [NN_WAVES][QT_P]
  int* wi = reinterpret_cast<int*>(wd + NN_WAVES * QT_P);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t chunk = blockIdx.x;
  const int tile = blockIdx.y;
  const int64_t TN = (int64_t)T * n;
  const double rsx = stdv[3 * root], rsy = stdv[3 * root + 1], rsz = stdv[3 * root + 2];
  const double rmx = mean[3 * root], rmy = mean[3 * root + 1], rmz = mean[3 * root + 2];
  for (int idx = threadIdx.x; idx < QT_P * TJ; idx += NN_THREADS) {
    const int qi = idx / TJ, m = idx - qi * TJ;
    const int t = m / J, k = m - t * J;
    const int64_t qg = (int64_t)tile * QT_P + qi;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (qg < Q) {
      const float* p = q + qg * TN + (int64_t)t * n;
      cx = nn_unnormalise(p[3 * k], stdv[3 * k], mean[3 * k], f32) - nn_unnormalise(p[3 * root], rsx, rmx, f32);
      cy = nn_unnormalise(p[3 * k + 1], stdv[3 * k + 1], mean[3 * k + 1], f32) - nn_unnormalise(p[3 * root + 1], rsy, rmy, f32);
      cz = nn_unnormalise(p[3 * k + 2], stdv[3 * k + 2], mean[3 * k + 2], f32) - nn_unnormalise(p[3 * root + 2], rsz, rmz, f32);
    }
    double* c = cq + (size_t)qi * 3 * TJ + m;
    c[0] = cx;
    c[TJ] = cy;
    c[2 * TJ] = cz;
  }
  __syncthreads();

  const int64_t r0 = chunk * VUNET_NN_CHUNK;
  const int64_t rend = r0 + VUNET_NN_CHUNK < (int64_t)N ? r0 + VUNET_NN_CHUNK : (int64_t)N;
  double bd = nn_inf();
  int bi = 0x7fffffff;
  for (int64_t r = r0 + wave; r < rend; r += NN_WAVES) {
    const float* row = bank + r * TN;
    double acc[QT_P];
#pragma unroll
    for (int qi = 0; qi < QT_P; ++qi) acc[qi] = 0.0;
    for (int m = lane; m < TJ; m += 64) {
      const int t = m / J, k = m - t * J;
      const float* p = row + (int64_t)t * n;
      const double jx = nn_unnormalise(p[3 * k], stdv[3 * k], mean[3 * k], f32) - nn_unnormalise(p[3 * root], rsx, rmx, f32);
      const double jy = nn_unnormalise(p[3 * k + 1], stdv[3 * k + 1], mean[3 * k + 1], f32) - nn_unnormalise(p[3 * root + 1], rsy, rmy, f32);
      const double jz = nn_unnormalise(p[3 * k + 2], stdv[3 * k + 2], mean[3 * k + 2], f32) - nn_unnormalise(p[3 * root + 2], rsz, rmz, f32);
#pragma unroll
      for (int qi = 0; qi < QT_P; ++qi) {
        const double* c = cq + (size_t)qi * 3 * TJ + m;
        const double dx = c[0] - jx, dy = c[TJ] - jy, dz = c[2 * TJ] - jz;
        acc[qi] += sqrt((dx * dx + dy * dy) + dz * dz);
      }
    }
#pragma unroll
    for (int qi = 0; qi < QT_P; ++qi) {
      const double d = nn_wave_sum(acc[qi]);
      if (lane == qi && nn_better(d, (int)r, bd, bi)) {
        bd = d;
        bi = (int)r;
      }
    }
  }
  nn_store_candidates<QT_P>(bd, bi, wd, wi, tile, Q, chunk, chunks, cand_d, cand_i);
}

// phase 2: a wave per query over its `chunks` candidates
__global__ __launch_bounds__(NN_THREADS) void nn_fold_kernel(const double* __restrict__ cand_d, const int* __restrict__ cand_i, int64_t chunks,
                                                             int Q, double* __restrict__ best_d, int* __restrict__ best_i) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t qg = (int64_t)blockIdx.x * NN_WAVES + wave;
  if (qg >= Q) return;
  const double* d = cand_d + qg * chunks;
  const int* i = cand_i + qg * chunks;
  double bd = nn_inf();
  int bi = 0x7fffffff;
  for (int64_t c = lane; c < chunks; c += 64) {
    const double od = d[c];
    const int oi = i[c];
    if (nn_better(od, oi, bd, bi)) {
      bd = od;
      bi = oi;
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const double od = __shfl_xor(bd, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (nn_better(od, oi, bd, bi)) {
      bd = od;
      bi = oi;
    }
  }
  if (lane == 0) {
    best_d[qg] = bd;
    best_i[qg] = bi;
  }
}

inline int64_t nn_chunks(int32_t N) { return ((int64_t)N + VUNET_NN_CHUNK - 1) / VUNET_NN_CHUNK; }

int nn_fold(void* scratch, int64_t chunks, int32_t Q, double* best_d, int32_t* best_i, hipStream_t stream) {
  const double* cand_d = (const double*)scratch;
  const int* cand_i = (const int*)(cand_d + (int64_t)Q * chunks);
  VUNET_LAUNCH(nn_fold_kernel, dim3((unsigned)((Q + NN_WAVES - 1) / NN_WAVES)), dim3(NN_THREADS), 0, stream, cand_d, cand_i, chunks, Q,
               best_d, best_i);
  return vunet_check_launch();
}

}  // namespace

extern "C" int vunet_nn_scratch_bytes(int32_t N, int32_t Q, int64_t* bytes) {
  if (!bytes || N < 1 || Q < 1) return VUNET_ERR_ARG;
  *bytes = nn_chunks(N) * Q * (int64_t)(sizeof(double) + sizeof(int32_t));
  return VUNET_OK;
}

extern "C" int vunet_nn_codes(const float* bank, int64_t ld, int32_t N, const float* q, int32_t Q, int32_t H, void* scratch,
                              double* best_d, int32_t* best_i, void* stream) {
  if (!bank || !q || !scratch || !best_d || !best_i || N < 1 || Q < 1 || H < 1 || ld < H || (uintptr_t)scratch % 8) return VUNET_ERR_ARG;
  const int64_t tiles = ((int64_t)Q + QT_C - 1) / QT_C;
  if (H > VUNET_NN_MAX_H || tiles > 65535) return VUNET_ERR_UNSUPPORTED;
  const int64_t chunks = nn_chunks(N);
  double* cand_d = (double*)scratch;
  int* cand_i = (int*)(cand_d + (int64_t)Q * chunks);
  const int Hp = (H + 255) / 256 * 256;
  const size_t lds = (size_t)QT_C * Hp * sizeof(float) + NN_WAVES * QT_C * (sizeof(double) + sizeof(int));
  const dim3 grid((unsigned)chunks, (unsigned)tiles), block(NN_THREADS);
  const bool vec = H % 4 == 0 && ld % 4 == 0 && (uintptr_t)bank % 16 == 0;
  if (lds > 64 * 1024) {
    const void* kern = vec ? (const void*)nn_codes_kernel<true> : (const void*)nn_codes_kernel<false>;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return VUNET_ERR_LAUNCH;
  }
  if (vec)
    VUNET_LAUNCH(nn_codes_kernel<true>, grid, block, lds, (hipStream_t)stream, bank, ld, N, q, Q, H, chunks, cand_d, cand_i);
  else
    VUNET_LAUNCH(nn_codes_kernel<false>, grid, block, lds, (hipStream_t)stream, bank, ld, N, q, Q, H, chunks, cand_d, cand_i);
  const int rc = vunet_check_launch();
  return rc ? rc : nn_fold(scratch, chunks, Q, best_d, best_i, (hipStream_t)stream);
}

extern "C" int vunet_nn_poses(const float* bank, int32_t N, const float* q, int32_t Q, int32_t T, int32_t J, int32_t root,
                              const double* mean, const double* stdv, int32_t f32_math, void* scratch, double* best_d, int32_t* best_i,
                              void* stream) {
  if (!bank || !q || !mean || !stdv || !scratch || !best_d || !best_i || N < 1 || Q < 1 || T < 1 || J < 1 || root < 0 || root >= J ||
      (uintptr_t)scratch % 8)
    return VUNET_ERR_ARG;
  const int64_t tiles = ((int64_t)Q + QT_P - 1) / QT_P;
  if ((int64_t)T * 3 * J > VUNET_NN_MAX_TN || tiles > 65535) return VUNET_ERR_UNSUPPORTED;
  const int64_t chunks = nn_chunks(N);
  double* cand_d = (double*)scratch;
  int* cand_i = (int*)(cand_d + (int64_t)Q * chunks);
  const size_t lds = (size_t)QT_P * 3 * T * J * sizeof(double) + NN_WAVES * QT_P * (sizeof(double) + sizeof(int));
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)nn_poses_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return VUNET_ERR_LAUNCH;
  VUNET_LAUNCH(nn_poses_kernel, dim3((unsigned)chunks, (unsigned)tiles), dim3(NN_THREADS), lds, (hipStream_t)stream, bank, N, q, Q, T, J,
               root, mean, stdv, f32_math ? 1 : 0, chunks, cand_d, cand_i);
  const int rc = vunet_check_launch();
  return rc ? rc : nn_fold(scratch, chunks, Q, best_d, best_i, (hipStream_t)stream);
}
