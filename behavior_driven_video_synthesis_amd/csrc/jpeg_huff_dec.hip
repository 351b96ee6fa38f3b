// Baseline JPEG entropy DEcoding on the device: the stuffed bytes of the scans -> the coefficients that the host walk
// (jpeg_entropy.h's entropy_decode) writes, bit for bit.  The C ABI is in include/vunet_jpeg_huffdec.h; the walk itself is
// jpeg_sync.h, shared with the host check (tools/jpeg_sync_check.cpp).
//
// A Huffman-coded segment (a scan, or one restart interval) is one bit string, but Huffman codes self-synchronise: a decoder started
// at an arbitrary bit soon falls into step with the true parse.  So a segment is cut into subsequences of VUNET_JPEG_SUBSEQ_BYTES,
// one thread each, and the serial walk becomes stages whose only hand-off between workgroups is the end of a launch:
//   sync    every thread walks its subsequence from its current entry state and proposes the entry state of the next one; double-
//           buffered (Jacobi), repeated inside a workgroup through LDS until nothing moves, and launch after launch across
//           workgroups until a device counter says that no state changed.  The first subsequence of a segment starts from a known
//           state, and each round fixes at least one more workgroup behind a fixed one: workgroups + 1 launches always suffice;
//   blocks  one workgroup per image: exclusive prefix sum of the blocks-begun counts within each segment -> block ordinals;
//   write   every thread walks again from its (now true) entry state and stores AC terms and DC differences into zeroed memory;
//           a block that straddles subsequences is written by several threads at disjoint k;
//   dc      the running sum of the DC differences per component in scan order, reset at every restart interval.
// One thread per subsequence diverges by nature: neighbouring lanes parse different symbols, and every lane reads its own bytes.
// The tables of a workgroup's image are brought into LDS once (5720 bytes).  No thread ever waits for another workgroup, every loop
// is bounded (jpeg_sync.h), and every index comes from rows that the entry point checked on their host copies before any launch.
#include "common.h"
#include "jpeg_huff_enc.h"
#include "jpeg_imgs.h"
#include "jpeg_sync.h"

namespace {

namespace S = vunet_jpeg_sync;

constexpr int kGroup = VUNET_JPEG_HUFFDEC_GROUP;
static_assert(sizeof(S::Tables) == VUNET_JPEG_HUFFDEC_TAB_BYTES && sizeof(S::Tables) % 4 == 0, "the table row is part of the ABI");
static_assert(sizeof(vunet_jpeg_subseq) == 40, "the subsequence row is part of the ABI");
static_assert(kGroup % 64 == 0 && kGroup <= 1024, "whole waves");

__constant__ uint8_t kZz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the words of `state` (VUNET_JPEG_HUFFDEC_STATE_WORDS per row)
struct Work {
  uint2* exits[2];   // the exit states of the rounds, alternating
  uint2* walked;     // the entry state each exit was walked from
  uint32_t* count;   // blocks begun
  uint32_t* prefix;  // their exclusive prefix sum over the image's rows
  uint32_t* ordinal; // the first block ordinal of each row
};

__host__ __device__ inline Work work_of(uint32_t* state, int64_t n) {
  Work w;
  w.exits[0] = reinterpret_cast<uint2*>(state);
  w.exits[1] = reinterpret_cast<uint2*>(state + 2 * n);
  w.walked = reinterpret_cast<uint2*>(state + 4 * n);
  w.count = state + 6 * n;
  w.prefix = state + 7 * n;
  w.ordinal = state + 8 * n;
  return w;
}

__device__ __forceinline__ void load_tables(const uint8_t* __restrict__ tabs, int img, S::Tables* T) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(tabs + (size_t)img * sizeof(S::Tables));
  uint32_t* dst = reinterpret_cast<uint32_t*>(T);
  for (int i = threadIdx.x; i < (int)(sizeof(S::Tables) / 4); i += kGroup) dst[i] = src[i];
}

__device__ __forceinline__ S::State state_of(uint2 v) { return S::State{v.x, v.y}; }
__device__ __forceinline__ uint2 words_of(S::State s) { return make_uint2(s.pos, s.at); }

__global__ __launch_bounds__(kGroup) void jpeg_huffdec_sync_kernel(const uint8_t* __restrict__ bytes,
                                                                   const vunet_jpeg_subseq* __restrict__ rows,
                                                                   const uint8_t* __restrict__ tabs, int64_t nsub,
                                                                   uint32_t* __restrict__ state, uint32_t* __restrict__ counter,
                                                                   int round) {
  __shared__ S::Tables T;
  __shared__ uint2 ex[kGroup];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * kGroup + t;
  const vunet_jpeg_subseq r = rows[i];
  load_tables(tabs, r.img, &T);   // (every row of a workgroup names the same image)
  const Work w = work_of(state, nsub);
  const uint2* rd = w.exits[round & 1];
  uint2* wr = w.exits[(round + 1) & 1];
  const bool pad = r.flags & VUNET_JPEG_SUBSEQ_PAD, first = r.flags & VUNET_JPEG_SUBSEQ_FIRST;
  // round 0 starts from the guess "every subsequence begins a block at its first bit" (the canonical lost state of the one before)
  S::State mine = {(uint32_t)r.end << 3, 0u}, walked = {0xFFFFFFFFu, 0xFFFFFFFFu}, from = {(uint32_t)r.begin << 3, 0u};
  uint32_t begun = 0;
  if (pad) mine = S::State{0u, 0u};
  if (round != 0 && !pad) {
    mine = state_of(rd[i]);
    walked = state_of(w.walked[i]);
    begun = w.count[i];
    if (!first && t == 0) from = state_of(rd[i - 1]);   // (the row before belongs to the same segment: checked on the host)
  }
  const S::State initial = mine;
  ex[t] = words_of(mine);
  __syncthreads();
  const S::Grid none = {1, 1, 1, 1, 1, 0, 0};
  for (int it = 0; it < kGroup; ++it) {
    const S::State entry = (first || t == 0) ? from : state_of(ex[t - 1]);
    bool changed = false;
    if (!pad && !S::same(entry, walked)) {
      const S::Result R = S::walk<false>(bytes, (uint32_t)r.seg_begin, (uint32_t)r.seg_end, entry, (uint32_t)r.end << 3, T, kZz, nullptr,
                                         none, 0u, 0u, 0u);
      walked = entry;
      begun = R.blocks;
      changed = !S::same(R.s, mine);
      mine = R.s;
    }
    __syncthreads();   // (every ex[t - 1] of this turn has been read)
    ex[t] = words_of(mine);
    if (!__syncthreads_or(changed)) break;
  }
  if (!pad) {
    wr[i] = words_of(mine);
    w.walked[i] = words_of(walked);
    w.count[i] = begun;
  }
  const int moved = __syncthreads_count(!pad && !S::same(mine, initial));
  if (t == 0 && moved) atomicAdd(counter, (uint32_t)moved);
}

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  return v;
}

// -> the sum of v over the threads before this one; *total: over all kGroup.  sums: LDS [kGroup / 64]  (jpeg_huff.hip's scan)
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* sums, uint32_t* total) {
  const uint32_t incl = wave_inclusive(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 63) sums[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < kGroup / 64; ++i) {
    before += i < wave ? sums[i] : 0u;
    all += sums[i];
  }
  *total = all;
  return before + incl - v;
}

// one workgroup per image
__global__ __launch_bounds__(kGroup) void jpeg_huffdec_blocks_kernel(const vunet_jpeg_subseq* __restrict__ rows,
                                                                     const int32_t* __restrict__ spans, int64_t nsub,
                                                                     uint32_t* __restrict__ state, uint32_t* __restrict__ flags) {
  __shared__ uint32_t sums[kGroup / 64];
  const Work w = work_of(state, nsub);
  const int64_t row0 = spans[2 * blockIdx.x];
  const int n = spans[2 * blockIdx.x + 1];
  uint32_t carry = 0;
  for (int base = 0; base < n; base += kGroup) {
    const int64_t i = row0 + base + threadIdx.x;   // (n is a multiple of kGroup)
    const uint32_t v = (rows[i].flags & VUNET_JPEG_SUBSEQ_PAD) ? 0u : w.count[i];
    uint32_t all;
    w.prefix[i] = carry + block_exclusive(v, sums, &all);
    carry += all;
  }
  __threadfence_block();
  __syncthreads();
  bool bad = false;
  for (int base = 0; base < n; base += kGroup) {
    const int64_t i = row0 + base + threadIdx.x;
    const vunet_jpeg_subseq r = rows[i];
    if (r.flags & VUNET_JPEG_SUBSEQ_PAD) continue;
    const uint32_t in_seg = w.prefix[i] - w.prefix[r.seg_row];   // (seg_row <= i, inside this image's rows: checked on the host)
    w.ordinal[i] = (uint32_t)r.first_block + in_seg;
    if (r.flags & VUNET_JPEG_SUBSEQ_LAST)
      bad |= S::segment_short(in_seg + w.count[i], (uint32_t)r.seg_blocks, (r.flags & VUNET_JPEG_SUBSEQ_TAIL) != 0);
  }
  if (bad) atomicOr(flags + blockIdx.x, (uint32_t)VUNET_JPEG_HUFFDEC_SHORT);
}

__global__ __launch_bounds__(kGroup) void jpeg_huffdec_write_kernel(const uint8_t* __restrict__ bytes,
                                                                    const vunet_jpeg_subseq* __restrict__ rows,
                                                                    const uint8_t* __restrict__ tabs,
                                                                    const vunet_jpeg_img* __restrict__ imgs, int64_t nsub,
                                                                    const uint32_t* __restrict__ state, int final_buffer,
                                                                    int16_t* __restrict__ coef, uint32_t* __restrict__ flags) {
  __shared__ S::Tables T;
  const int64_t i = (int64_t)blockIdx.x * kGroup + threadIdx.x;
  const vunet_jpeg_subseq r = rows[i];
  load_tables(tabs, r.img, &T);
  __syncthreads();
  if (r.flags & VUNET_JPEG_SUBSEQ_PAD) return;
  const Work w = work_of(const_cast<uint32_t*>(state), nsub);
  const bool first = r.flags & VUNET_JPEG_SUBSEQ_FIRST, tail = r.flags & VUNET_JPEG_SUBSEQ_TAIL;
  const S::State entry = first ? S::State{(uint32_t)r.begin << 3, 0u} : state_of(w.exits[final_buffer][i - 1]);
  const vunet_jpeg_img im = imgs[r.img];
  const S::Grid g = {T.per_mcu, im.hsamp, im.vsamp, im.bw0 / im.hsamp, im.bw0, im.bw0 * im.bh0, im.bw1 * im.bh1};
  const uint32_t nblocks = (uint32_t)(g.n0 + 2 * g.n1), lo = (uint32_t)r.first_block;
  uint32_t hi = lo + (uint32_t)r.seg_blocks;
  hi = hi < nblocks ? hi : nblocks;
  const S::Result R = S::walk<true>(bytes, (uint32_t)r.seg_begin, (uint32_t)r.seg_end, entry, (uint32_t)r.end << 3, T, kZz,
                                    coef + im.coef_off, g, w.ordinal[i], lo, hi);
  if (S::write_refused(R, (r.flags & VUNET_JPEG_SUBSEQ_LAST) != 0, tail)) atomicOr(flags + r.img, (uint32_t)VUNET_JPEG_HUFFDEC_ERROR);
}

// grid (N, 3): one workgroup per component of an image; a segmented inclusive scan of its DC terms in scan order
__global__ __launch_bounds__(kGroup) void jpeg_huffdec_dc_kernel(const vunet_jpeg_img* __restrict__ imgs, const uint8_t* __restrict__ tabs,
                                                                 int16_t* __restrict__ coef) {
  __shared__ uint32_t wave_v[kGroup / 64];
  __shared__ uint32_t wave_f[kGroup / 64];
  const vunet_jpeg_img im = imgs[blockIdx.x];
  const int c = blockIdx.y;
  if (c >= im.ncomp) return;
  const int restart = reinterpret_cast<const S::Tables*>(tabs + (size_t)blockIdx.x * sizeof(S::Tables))->restart;
  const int hs = im.hsamp, vs = im.vsamp, hv = c == 0 ? hs * vs : 1, cols = im.bw0 / hs;
  const int n0 = im.bw0 * im.bh0, n1 = im.bw1 * im.bh1, n = c == 0 ? n0 : n1;
  int16_t* base = coef + im.coef_off;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int start = 0; start < n; start += kGroup) {
    const int j = start + threadIdx.x;
    uint32_t v = 0, f = 0;
    int64_t at = 0;
    if (j < n) {
      const int m = j / hv, r = j % hv;   // the MCU and the block's place in it
      at = c == 0 ? ((int64_t)((m / cols) * vs + r / hs) * im.bw0 + (m % cols) * hs + r % hs) * 64 : ((int64_t)n0 + (int64_t)(c - 1) * n1 + j) * 64;
      v = (uint32_t)(int32_t)base[at];
      f = (j == 0 || (restart > 0 && r == 0 && m % restart == 0)) ? 1u : 0u;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t tv = __shfl_up(v, d, 64), tf = __shfl_up(f, d, 64);
      if (lane >= d) {
        if (!f) v += tv;
        f |= tf;
      }
    }
    __syncthreads();   // (the sums of the turn before have been read)
    if (lane == 63) {
      wave_v[wave] = v;
      wave_f[wave] = f;
    }
    __syncthreads();
    uint32_t cv = carry, av = carry;   // the running sum in front of this wave; `av`: in front of the next turn
#pragma unroll
    for (int k = 0; k < kGroup / 64; ++k) {
      av = wave_f[k] ? wave_v[k] : av + wave_v[k];
      if (k + 1 == wave) cv = av;
    }
    if (j < n) base[at] = (int16_t)(uint16_t)(f ? v : cv + v);
    carry = av;
  }
}

bool common_ok(const vunet_jpeg_subseq* rows, const vunet_jpeg_subseq* rows_host, int64_t nsub, const vunet_jpeg_img* imgs_host,
               int32_t N, int64_t bytes_count, int64_t coef_count, const void* state, int64_t state_count) {
  int64_t total = 0;
  return rows && rows_host && imgs_host && state && N >= 1 && N <= 65535 && vunet_jpeg::aligned16(state) &&
         vunet_jpeg::imgs_ok(imgs_host, N, coef_count, INT64_MAX, INT64_MAX, 65535, 65535, 65535, &total) &&
         vunet_jpeg::grids_exact(imgs_host, N, 0) && vunet_jpeg::subseq_rows_ok(rows_host, nsub, bytes_count, imgs_host, N) &&
         state_count >= nsub * VUNET_JPEG_HUFFDEC_STATE_WORDS;
}

bool spans_cover(const int32_t* spans_host, const vunet_jpeg_subseq* rows_host, int64_t nsub, int32_t N) {
  int64_t at = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t row0 = spans_host[2 * n], count = spans_host[2 * n + 1];
    if (row0 != at || count < 0 || count % kGroup || at + count > nsub) return false;
    for (int64_t i = row0; i < row0 + count; i += kGroup)
      if (rows_host[i].img != n) return false;   // (a workgroup's rows name one image: subseq_rows_ok)
    at += count;
  }
  return at == nsub;
}

}  // namespace

extern "C" int vunet_jpeg_scan_segments(const uint8_t* bytes, int64_t len, const vunet_jpeg_info* info, int64_t* segs, int64_t seg_cap,
                                        int64_t* nseg, uint16_t* qtab, uint8_t* tab) {
  return vunet_jpeg::scan_segments(bytes, len, info, segs, seg_cap, nseg, qtab, tab);
}

extern "C" int vunet_jpeg_huffdec_rows(const int64_t* segs, int64_t nseg, const vunet_jpeg_info* info, int32_t img, int64_t byte_off,
                                       int64_t row0, vunet_jpeg_subseq* rows, int64_t row_cap, int64_t* nrows) {
  return vunet_jpeg::subseq_rows(segs, nseg, info, img, byte_off, row0, rows, row_cap, nrows);
}

extern "C" int vunet_jpeg_huffdec_sync(const uint8_t* bytes, int64_t bytes_count, const vunet_jpeg_subseq* rows,
                                       const vunet_jpeg_subseq* rows_host, int64_t nsub, const uint8_t* tabs, const uint8_t* tabs_host,
                                       const vunet_jpeg_img* imgs_host, int32_t N, uint32_t* state, int64_t state_count,
                                       uint32_t* counters, int64_t counters_count, int32_t first, int32_t launches, void* stream) {
  if (!bytes || !tabs || !tabs_host || !counters || first < 0 || launches < 1 || (int64_t)first + launches > counters_count ||
      !vunet_jpeg::aligned16(tabs) || !common_ok(rows, rows_host, nsub, imgs_host, N, bytes_count, INT64_MAX, state, state_count) ||
      !vunet_jpeg::table_rows_ok(tabs_host, imgs_host, N))
    return VUNET_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counters + first, 0, (size_t)launches * sizeof(uint32_t), s) != hipSuccess) return VUNET_ERR_LAUNCH;
  for (int l = first; l < first + launches; ++l)
    VUNET_LAUNCH(jpeg_huffdec_sync_kernel, dim3((unsigned)(nsub / kGroup)), dim3(kGroup), 0, s, bytes, rows, tabs, nsub, state,
                 counters + l, l);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huffdec_blocks(const vunet_jpeg_subseq* rows, const vunet_jpeg_subseq* rows_host, int64_t nsub,
                                         const int32_t* spans, const int32_t* spans_host, const vunet_jpeg_img* imgs_host, int32_t N,
                                         uint32_t* state, int64_t state_count, uint32_t* flags, int64_t flags_count, void* stream) {
  if (!spans || !spans_host || !flags || flags_count < N ||
      !common_ok(rows, rows_host, nsub, imgs_host, N, VUNET_JPEG_HUFFDEC_MAX_BYTES, INT64_MAX, state, state_count) ||
      !spans_cover(spans_host, rows_host, nsub, N))
    return VUNET_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(flags, 0, (size_t)N * sizeof(uint32_t), s) != hipSuccess) return VUNET_ERR_LAUNCH;
  VUNET_LAUNCH(jpeg_huffdec_blocks_kernel, dim3((unsigned)N), dim3(kGroup), 0, s, rows, spans, nsub, state, flags);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huffdec_write(const uint8_t* bytes, int64_t bytes_count, const vunet_jpeg_subseq* rows,
                                        const vunet_jpeg_subseq* rows_host, int64_t nsub, const uint8_t* tabs, const uint8_t* tabs_host,
                                        const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, const uint32_t* state,
                                        int64_t state_count, int32_t rounds_final, int16_t* coef, int64_t coef_count, uint32_t* flags,
                                        int64_t flags_count, void* stream) {
  if (!bytes || !tabs || !tabs_host || !imgs || !coef || !flags || flags_count < N || rounds_final < 1 || coef_count < 0 ||
      !vunet_jpeg::aligned16(tabs) || !vunet_jpeg::aligned16(coef) ||
      !common_ok(rows, rows_host, nsub, imgs_host, N, bytes_count, coef_count, state, state_count) ||
      !vunet_jpeg::table_rows_ok(tabs_host, imgs_host, N))
    return VUNET_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(coef, 0, (size_t)coef_count * sizeof(int16_t), s) != hipSuccess) return VUNET_ERR_LAUNCH;
  // round L writes exits[(L + 1) & 1]: after `rounds_final` rounds the last one written is exits[rounds_final & 1]
  VUNET_LAUNCH(jpeg_huffdec_write_kernel, dim3((unsigned)(nsub / kGroup)), dim3(kGroup), 0, s, bytes, rows, tabs, imgs, nsub, state,
               (int)(rounds_final & 1), coef, flags);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huffdec_dc(const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, const uint8_t* tabs,
                                     const uint8_t* tabs_host, int32_t N, int16_t* coef, int64_t coef_count, void* stream) {
  int64_t total = 0;
  if (!imgs || !imgs_host || !tabs || !tabs_host || !coef || N < 1 || N > 65535 || coef_count < 0 || !vunet_jpeg::aligned16(tabs) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, coef_count, INT64_MAX, INT64_MAX, 65535, 65535, 65535, &total) ||
      !vunet_jpeg::grids_exact(imgs_host, N, 0) || !vunet_jpeg::table_rows_ok(tabs_host, imgs_host, N))
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(jpeg_huffdec_dc_kernel, dim3((unsigned)N, 3u), dim3(kGroup), 0, (hipStream_t)stream, imgs, tabs, coef);
  return vunet_check_launch();
}
