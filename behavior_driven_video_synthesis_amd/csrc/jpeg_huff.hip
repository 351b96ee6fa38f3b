// Baseline JPEG entropy coding on the device: the quantised coefficients vunet_jpeg_fdct leaves -> the scan's bytes, stuffed, ready
// to stand between the header and EOI that the host writes (jpeg_huff_enc.h).  The C ABI is in include/vunet_jpeg_enc.h.
//
// The unit is the 8 x 8 block: its symbols, code lengths and bits depend on its 64 coefficients and one neighbouring DC value, whose
// place has a closed form (the previous block of the component in scan order).  So the serial bit walk of the host coder becomes
// stages whose only hand-off between workgroups is the end of a launch -- nothing inside a launch waits for another workgroup:
//   count    (optimised tables only) per-image symbol histograms, integer atomic adds on zeroed memory;
//   lengths  per block in scan order its bit count under its image's tables; the range check sets a per-image word;
//   scan     one workgroup per image: exclusive prefix sum -> every block's bit offset, the image's bit total;
//   pack     every block's bits to their offset in the image's unstuffed stream (big-endian words, atomic OR on zeroed memory:
//            neighbouring blocks share words), the last byte padded with 1-bits;
//   stuff    per 1024-byte chunk the bytes it will take (one more per 0xFF), a one-workgroup prefix sum over the chunks of the
//            whole batch, then every byte to its final place: the batch's scans lie end to end, and only they are downloaded.
// Integer add and OR commute, so no result depends on the dispatch order.  One thread per block; a workgroup's 256 blocks are
// first brought into LDS with coalesced 16-byte loads (rows of 33 words: the lanes of a wave read one zigzag position of 64
// different blocks from 64 different banks), then every thread walks its block exactly as jpeg_huff_enc.h's walk_blocks does.
// Every store is bounded by what the entry point checked on the host copies of the rows, table rows and spans (VUNET_ERR_ARG
// otherwise); the pack and stuff kernels bound their own stores as well, since the spans come from the device's own sums.
// No allocation and no synchronisation in here: every entry point is recordable in a hipGraph.
#include "common.h"
#include "jpeg_huff_enc.h"
#include "jpeg_imgs.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowWords = 33;
constexpr int kChunk = (int)vunet_jpeg::kStuffChunk;   // 256 threads x one word

__constant__ uint8_t kZz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// block g of the batch, counted in scan order image after image
struct Where {
  int img, chroma, last;   // its image; 0: luma tables, 1: chroma tables; the image's last block
  int64_t off, pred;       // its coefficients and those of its DC predecessor, in elements of `coef` (pred -1: none)
};

__device__ __forceinline__ Where locate(const vunet_jpeg_img* __restrict__ imgs, int N, int g) {
  int lo = 0, hi = N - 1;   // the last image whose first block is <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (imgs[mid].block0 <= g) lo = mid; else hi = mid - 1;
  }
  const vunet_jpeg_img im = imgs[lo];
  const int s = g - im.block0, n0 = im.bw0 * im.bh0, n1 = im.bw1 * im.bh1;
  const int hs = im.hsamp, vs = im.vsamp, hv = hs * vs, per_mcu = im.ncomp == 3 ? hv + 2 : 1, cols = im.bw0 / hs;
  const int m = s / per_mcu, r = s % per_mcu, my = m / cols, mx = m % cols;
  Where w;
  w.img = lo;
  w.last = s == n0 + 2 * n1 - 1;
  int idx, pidx = -1;
  if (r < hv) {   // luma: row-major inside the MCU; before its first block comes the last one of the MCU before
    w.chroma = 0;
    idx = (my * vs + r / hs) * im.bw0 + mx * hs + r % hs;
    if (r > 0) pidx = (my * vs + (r - 1) / hs) * im.bw0 + mx * hs + (r - 1) % hs;
    else if (m > 0) pidx = (((m - 1) / cols) * vs + vs - 1) * im.bw0 + ((m - 1) % cols) * hs + hs - 1;
  } else {        // chroma: one block per MCU, the planes are in MCU order
    w.chroma = 1;
    idx = n0 + (r - hv) * n1 + m;
    if (m > 0) pidx = idx - 1;
  }
  w.off = (int64_t)im.coef_off + (int64_t)idx * 64;
  w.pred = pidx < 0 ? -1 : (int64_t)im.coef_off + (int64_t)pidx * 64;
  return w;
}

// the workgroup's blocks into LDS: block b's 64 coefficients (natural order) from rows + b * kRowWords.  off < 0: no block
__device__ __forceinline__ void stage(const int16_t* __restrict__ coef, int64_t off, uint32_t* rows, int64_t* offs) {
  offs[threadIdx.x] = off;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int i = threadIdx.x + kThreads * r, b = i >> 3, part = i & 7;
    const int64_t o = offs[b];
    if (o >= 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(coef + o + part * 8);
      uint32_t* d = rows + b * kRowWords + part * 4;
      d[0] = v.x;
      d[1] = v.y;
      d[2] = v.z;
      d[3] = v.w;
    }
  }
  __syncthreads();
}

// jpeg_huff_enc.h's walk of one block: f(table 0 DC / 1 AC, symbol, the value's bits, their count).  -> false: out of range
template <class F>
__device__ __forceinline__ bool walk(const int16_t* blk, int pred, F& f) {
  const int diff = (int)blk[0] - pred;
  int nb = 32 - __clz(diff < 0 ? -diff : diff);
  if (nb > 11) return false;
  f(0, nb, (uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int v = blk[kZz[k]];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) f(1, 0xF0, 0u, 0);
    nb = 32 - __clz(v < 0 ? -v : v);
    if (nb > 10) return false;
    f(1, (run << 4) | nb, (uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1), nb);
    run = 0;
  }
  if (run) f(1, 0x00, 0u, 0);
  return true;
}

struct Count {
  uint32_t* hist;   // [2][256]: the component's DC and AC rows, in LDS or in global memory
  __device__ __forceinline__ void operator()(int t, int sym, uint32_t, int) { atomicAdd(hist + 256 * t + sym, 1u); }
};

struct Length {
  const uint32_t* tab;   // [2][256]
  uint32_t bits;
  bool missing;
  __device__ __forceinline__ void operator()(int t, int sym, uint32_t, int nb) {
    const uint32_t cw = tab[256 * t + sym];
    missing |= cw == 0;
    bits += (cw >> 16) + nb;
  }
};

// bits into big-endian 32-bit words from bit `at` of `words`; words at or beyond `limit` are dropped
struct Pack {
  const uint32_t* tab;
  uint32_t* words;
  uint32_t w, limit;
  uint64_t acc;   // the low n bits wait; n < 32 between calls, the first word's bits in front of `at` count as zeros
  int n;
  __device__ __forceinline__ void flush(uint32_t x) {
    if (x != 0 && w < limit) atomicOr(words + w, __builtin_bswap32(x));
    ++w;
  }
  __device__ __forceinline__ void push(uint32_t code, int len) {   // len <= 27
    acc = (acc << len) | code;
    n += len;
    if (n >= 32) {
      n -= 32;
      flush((uint32_t)(acc >> n));
    }
  }
  __device__ __forceinline__ void operator()(int t, int sym, uint32_t extra, int nb) {
    const uint32_t cw = tab[256 * t + sym];
    push(((cw & 0xFFFFu) << nb) | extra, (int)(cw >> 16) + nb);
  }
  __device__ __forceinline__ void finish(bool pad) {   // pad: 1-bits up to the next byte
    const int p = (8 - (n & 7)) & 7;
    if (pad && p) push((1u << p) - 1, p);
    if (n) flush((uint32_t)(acc << (32 - n)));
  }
};

__global__ __launch_bounds__(kThreads) void jpeg_zero_kernel(uint4* __restrict__ p, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kThreads)
    p[i] = make_uint4(0, 0, 0, 0);
}

__global__ __launch_bounds__(kThreads) void jpeg_huff_count_kernel(const int16_t* __restrict__ coef,
                                                                   const vunet_jpeg_img* __restrict__ imgs, int N, int total,
                                                                   uint32_t* __restrict__ hist) {
  __shared__ uint32_t rows[kThreads * kRowWords];
  __shared__ int64_t offs[kThreads];
  __shared__ uint32_t local[4 * 256];   // the histogram of the image the workgroup's first block belongs to
  __shared__ int first_img;
  const int g = blockIdx.x * kThreads + threadIdx.x;
  Where w;
  w.off = -1;
  w.img = -1;
  if (g < total) w = locate(imgs, N, g);
  if (threadIdx.x == 0) first_img = w.img;   // (block 0 of a workgroup always exists)
#pragma unroll
  for (int i = 0; i < 4; ++i) local[threadIdx.x + kThreads * i] = 0u;
  stage(coef, w.off, rows, offs);            // (its barriers order the stores above, too)
  if (g < total) {
    // a few hot symbols take most of the counts: they meet in LDS, and global memory sees one add per symbol and workgroup.
    // Blocks of a later image in the same workgroup (small images) add to global memory directly
    const int16_t* blk = reinterpret_cast<const int16_t*>(rows + threadIdx.x * kRowWords);
    const int pred = w.pred < 0 ? 0 : (int)coef[w.pred];
    if (w.img == first_img) {   // (two walks, so that each knows its address space: LDS adds here, global ones there)
      Count f{local + 2 * w.chroma * 256};
      walk(blk, pred, f);
    } else {
      Count f{hist + ((size_t)w.img * 4 + 2 * w.chroma) * 256};
      walk(blk, pred, f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t v = local[threadIdx.x + kThreads * i];
    if (v) atomicAdd(hist + (size_t)first_img * 1024 + threadIdx.x + kThreads * i, v);
  }
}

__global__ __launch_bounds__(kThreads) void jpeg_huff_lengths_kernel(const int16_t* __restrict__ coef,
                                                                     const vunet_jpeg_img* __restrict__ imgs, int N, int total,
                                                                     const uint32_t* __restrict__ codes,
                                                                     const int32_t* __restrict__ tab_row, uint32_t* __restrict__ bits,
                                                                     uint32_t* __restrict__ status) {
  __shared__ uint32_t rows[kThreads * kRowWords];
  __shared__ int64_t offs[kThreads];
  const int g = blockIdx.x * kThreads + threadIdx.x;
  Where w;
  w.off = -1;
  if (g < total) w = locate(imgs, N, g);
  stage(coef, w.off, rows, offs);
  if (g >= total) return;
  Length f{codes + ((size_t)tab_row[w.img] * 4 + 2 * w.chroma) * 256, 0u, false};
  const bool ok = walk(reinterpret_cast<const int16_t*>(rows + threadIdx.x * kRowWords), w.pred < 0 ? 0 : (int)coef[w.pred], f);
  bits[g] = ok ? f.bits : 0u;
  if (!ok) status[2 * w.img] = 1u;             // every writer stores the same value
  if (f.missing) status[2 * w.img + 1] = 1u;
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

// -> the sum of v over the threads before this one; *total: over all kThreads.  sums: LDS [kThreads / 64]
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* sums, uint32_t* total) {
  const uint32_t incl = wave_inclusive(v);
  const int wave = threadIdx.x >> 6;
  __syncthreads();   // (the sums of the call before have been read)
  if ((threadIdx.x & 63) == 63) sums[wave] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < kThreads / 64; ++i) {
    before += i < wave ? sums[i] : 0u;
    all += sums[i];
  }
  *total = all;
  return before + incl - v;
}

// one workgroup per image: its blocks' bit counts -> bit offsets, in place; totals[image] = the sum.  Four blocks per thread and turn
__global__ __launch_bounds__(kThreads) void jpeg_huff_scan_kernel(const vunet_jpeg_img* __restrict__ imgs, uint32_t* __restrict__ bits,
                                                                  uint32_t* __restrict__ totals) {
  __shared__ uint32_t sums[kThreads / 64];
  const vunet_jpeg_img im = imgs[blockIdx.x];
  const int n = im.bw0 * im.bh0 + 2 * im.bw1 * im.bh1;
  uint32_t* b = bits + im.block0;
  uint32_t carry = 0;
  for (int base = 0; base < n; base += 4 * kThreads) {
    const int i0 = base + 4 * threadIdx.x;
    uint32_t v[4], mine = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[j] = i0 + j < n ? b[i0 + j] : 0u;
      mine += v[j];
    }
    uint32_t all;
    uint32_t at = carry + block_exclusive(mine, sums, &all);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (i0 + j < n) b[i0 + j] = at;
      at += v[j];
    }
    carry += all;
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

__global__ __launch_bounds__(kThreads) void jpeg_huff_pack_kernel(const int16_t* __restrict__ coef,
                                                                  const vunet_jpeg_img* __restrict__ imgs, int N, int total,
                                                                  const uint32_t* __restrict__ codes,
                                                                  const int32_t* __restrict__ tab_row,
                                                                  const uint32_t* __restrict__ bitoff,
                                                                  const int64_t* __restrict__ spans, uint8_t* __restrict__ raw) {
  __shared__ uint32_t rows[kThreads * kRowWords];
  __shared__ int64_t offs[kThreads];
  const int g = blockIdx.x * kThreads + threadIdx.x;
  Where w;
  w.off = -1;
  if (g < total) w = locate(imgs, N, g);
  stage(coef, w.off, rows, offs);
  if (g >= total) return;
  const int64_t bytes = (spans[2 * w.img + 1] + 7) >> 3;
  const uint32_t at = bitoff[g];
  Pack f{codes + ((size_t)tab_row[w.img] * 4 + 2 * w.chroma) * 256,
         reinterpret_cast<uint32_t*>(raw + spans[2 * w.img]),
         at >> 5,
         (uint32_t)((bytes + kChunk - 1) / kChunk * (kChunk / 4)),
         0ull,
         (int)(at & 31)};
  walk(reinterpret_cast<const int16_t*>(rows + threadIdx.x * kRowWords), w.pred < 0 ? 0 : (int)coef[w.pred], f);
  f.finish(w.last != 0);
}

// chunk c of the batch's unstuffed bytes: this thread's word of it, and how many of its four bytes belong to the image's scan
__device__ __forceinline__ uint32_t chunk_word(const uint8_t* __restrict__ raw, const int64_t* __restrict__ spans, int N, int64_t c,
                                               int* valid, int* first) {
  int lo = 0, hi = N - 1;   // the last image that starts at or before the chunk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (spans[2 * mid] <= c * kChunk) lo = mid; else hi = mid - 1;
  }
  const int64_t at = c * kChunk + 4 * (int64_t)threadIdx.x, left = spans[2 * lo] + ((spans[2 * lo + 1] + 7) >> 3) - at;
  *valid = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  *first = spans[2 * lo] == c * kChunk ? lo : -1;
  return *reinterpret_cast<const uint32_t*>(raw + at);
}

__device__ __forceinline__ uint32_t stuffed_size(uint32_t word, int valid) {
  uint32_t n = (uint32_t)valid;
#pragma unroll
  for (int j = 0; j < 4; ++j) n += (j < valid && ((word >> (8 * j)) & 0xFF) == 0xFF) ? 1u : 0u;
  return n;
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_count_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ spans,
                                                                    int N, uint32_t* __restrict__ chunk_off) {
  __shared__ uint32_t sums[kThreads / 64];
  int valid, first;
  const uint32_t word = chunk_word(raw, spans, N, blockIdx.x, &valid, &first);
  uint32_t all;
  block_exclusive(stuffed_size(word, valid), sums, &all);
  if (threadIdx.x == 0) chunk_off[blockIdx.x] = all;
}

// one workgroup: the chunks' sizes -> their offsets in `out`, in place; *total = the batch's bytes
__global__ __launch_bounds__(kThreads) void jpeg_stuff_scan_kernel(uint32_t* __restrict__ chunk_off, int nchunks,
                                                                   uint32_t* __restrict__ total) {
  __shared__ uint32_t sums[kThreads / 64];
  uint32_t carry = 0;
  for (int base = 0; base < nchunks; base += kThreads) {
    const int i = base + threadIdx.x;
    const uint32_t v = i < nchunks ? chunk_off[i] : 0u;
    uint32_t all;
    const uint32_t at = carry + block_exclusive(v, sums, &all);
    if (i < nchunks) chunk_off[i] = at;
    carry += all;
  }
  if (threadIdx.x == 0) *total = carry;
}

__global__ __launch_bounds__(kThreads) void jpeg_stuff_write_kernel(const uint8_t* __restrict__ raw, const int64_t* __restrict__ spans,
                                                                    int N, const uint32_t* __restrict__ chunk_off,
                                                                    uint8_t* __restrict__ out, int64_t out_cap,
                                                                    uint32_t* __restrict__ img_start) {
  __shared__ uint32_t sums[kThreads / 64];
  int valid, first;
  const uint32_t word = chunk_word(raw, spans, N, blockIdx.x, &valid, &first);
  uint32_t all;
  int64_t at = (int64_t)chunk_off[blockIdx.x] + block_exclusive(stuffed_size(word, valid), sums, &all);
  if (threadIdx.x == 0 && first >= 0) img_start[first] = chunk_off[blockIdx.x];
  for (int j = 0; j < valid; ++j) {
    const uint32_t b = (word >> (8 * j)) & 0xFF;
    if (at < out_cap) out[at] = (uint8_t)b;
    ++at;
    if (b == 0xFF) {
      if (at < out_cap) out[at] = 0;
      ++at;
    }
  }
}

// the rows against the coefficients, the table rows against the code tables: -> the batch's blocks, or -1
int64_t coder_args_ok(const void* coef, int64_t coef_count, const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N) {
  int64_t total = 0;
  if (!coef || !imgs || !imgs_host || N < 1 || N > 65535 || coef_count < 0 || !vunet_jpeg::aligned16(coef) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, coef_count, INT64_MAX, INT64_MAX, 65535, 65535, 65535, &total) ||
      !vunet_jpeg::grids_exact(imgs_host, N, 0))
    return -1;
  return total;
}

bool tables_ok(const void* codes, int64_t code_rows, const void* tab_row, const int32_t* tab_row_host, int32_t N) {
  if (!codes || !tab_row || !tab_row_host || code_rows < 1) return false;
  for (int n = 0; n < N; ++n)
    if (tab_row_host[n] < 0 || tab_row_host[n] >= code_rows) return false;
  return true;
}

unsigned groups_of(int64_t count, int per) { return (unsigned)((count + per - 1) / per); }

void zero(void* p, int64_t bytes, hipStream_t stream) {   // bytes: a multiple of 16
  const int64_t count = bytes / 16;
  const unsigned groups = groups_of(count, kThreads);
  VUNET_LAUNCH(jpeg_zero_kernel, dim3(groups < 2048u ? groups : 2048u), dim3(kThreads), 0, stream, reinterpret_cast<uint4*>(p), count);
}

}  // namespace

extern "C" int vunet_jpeg_huff_count(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs,
                                     const vunet_jpeg_img* imgs_host, int32_t N, uint32_t* hist, int64_t hist_count, void* stream) {
  const int64_t total = coder_args_ok(coef, coef_count, imgs, imgs_host, N);
  if (total < 0 || !hist || !vunet_jpeg::aligned16(hist) || hist_count < (int64_t)N * 1024) return VUNET_ERR_ARG;
  zero(hist, (int64_t)N * 4096, (hipStream_t)stream);
  VUNET_LAUNCH(jpeg_huff_count_kernel, dim3(groups_of(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, coef, imgs, (int)N,
               (int)total, hist);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huff_lengths(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs,
                                       const vunet_jpeg_img* imgs_host, int32_t N, const uint32_t* codes, int64_t code_rows,
                                       const int32_t* tab_row, const int32_t* tab_row_host, uint32_t* bits, int64_t bits_count,
                                       uint32_t* totals, int64_t totals_count, void* stream) {
  const int64_t total = coder_args_ok(coef, coef_count, imgs, imgs_host, N);
  if (total < 0 || !tables_ok(codes, code_rows, tab_row, tab_row_host, N) || !bits || !totals || !vunet_jpeg::aligned16(totals) ||
      bits_count < total || totals_count < (N + 3) / 4 * 4 + (2 * (int64_t)N + 3) / 4 * 4)
    return VUNET_ERR_ARG;
  uint32_t* status = totals + (N + 3) / 4 * 4;   // totals: [round_up(N, 4)] sums, then [N][2] status words, zeroed here
  zero(status, ((int64_t)N * 8 + 15) / 16 * 16, (hipStream_t)stream);
  VUNET_LAUNCH(jpeg_huff_lengths_kernel, dim3(groups_of(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, coef, imgs, (int)N,
               (int)total, codes, tab_row, bits, status);
  VUNET_LAUNCH(jpeg_huff_scan_kernel, dim3((unsigned)N), dim3(kThreads), 0, (hipStream_t)stream, imgs, bits, totals);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huff_pack(const int16_t* coef, int64_t coef_count, const vunet_jpeg_img* imgs,
                                    const vunet_jpeg_img* imgs_host, int32_t N, const uint32_t* codes, int64_t code_rows,
                                    const int32_t* tab_row, const int32_t* tab_row_host, const uint32_t* bitoff, int64_t bits_count,
                                    const int64_t* spans, const int64_t* spans_host, uint8_t* raw, int64_t raw_bytes, void* stream) {
  const int64_t total = coder_args_ok(coef, coef_count, imgs, imgs_host, N);
  int64_t nchunks = 0;
  if (total < 0 || !tables_ok(codes, code_rows, tab_row, tab_row_host, N) || !bitoff || bits_count < total || !spans || !spans_host ||
      !raw || !vunet_jpeg::aligned16(raw) || raw_bytes < 0 ||
      !vunet_jpeg::spans_ok(spans_host, imgs_host, N, raw_bytes, INT64_MAX, INT64_MAX, &nchunks))
    return VUNET_ERR_ARG;
  zero(raw, nchunks * kChunk, (hipStream_t)stream);
  VUNET_LAUNCH(jpeg_huff_pack_kernel, dim3(groups_of(total, kThreads)), dim3(kThreads), 0, (hipStream_t)stream, coef, imgs, (int)N,
               (int)total, codes, tab_row, bitoff, spans, raw);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_huff_stuff(const uint8_t* raw, int64_t raw_bytes, const vunet_jpeg_img* imgs_host, const int64_t* spans,
                                     const int64_t* spans_host, int32_t N, uint32_t* chunk_off, int64_t chunk_count, uint8_t* out,
                                     int64_t out_cap, uint32_t* img_start, void* stream) {
  int64_t total = 0, nchunks = 0;
  if (!raw || !imgs_host || !spans || !spans_host || !chunk_off || !out || !img_start || N < 1 || N > 65535 || raw_bytes < 0 ||
      out_cap < 0 || chunk_count < 0 || !vunet_jpeg::aligned16(raw) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, INT64_MAX, INT64_MAX, INT64_MAX, 65535, 65535, 65535, &total) ||
      !vunet_jpeg::spans_ok(spans_host, imgs_host, N, raw_bytes, out_cap, chunk_count, &nchunks) || nchunks > 0x7FFFFFFF)
    return VUNET_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  VUNET_LAUNCH(jpeg_stuff_count_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, raw, spans, (int)N, chunk_off);
  VUNET_LAUNCH(jpeg_stuff_scan_kernel, dim3(1), dim3(kThreads), 0, s, chunk_off, (int)nchunks, img_start + N);
  VUNET_LAUNCH(jpeg_stuff_write_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, raw, spans, (int)N, chunk_off, out, out_cap,
               img_start);
  return vunet_check_launch();
}
