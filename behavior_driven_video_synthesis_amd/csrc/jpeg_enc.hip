// Baseline JPEG encode: the C ABI of include/vunet_jpeg_enc.h.  The mirror image of jpeg.hip: the device half is here -- RGB ->
// YCbCr with libjpeg's chroma down-sampling and edge padding, then the level shift, libjpeg's integer "islow" forward DCT and the
// quantiser into the decoder's coefficient layout -- and the host half (tables, segments, Huffman coder) is jpeg_huff_enc.h and
// calls no HIP.  Two launches per batch, whatever the images' sizes and samplings: one vunet_jpeg_img row per image says where its
// pixels, planes, tables and coefficients lie.
//
// The reference writes every frame with cv2.VideoWriter / cv2.imwrite on the host (lib/logging.py, lib/figures.py), i.e. through
// libjpeg-turbo's default encoder; the rules restated from jccolor.c, jcsample.c, jcprepct.c, jfdctint.c, jcdctmgr.c and jccoefct.c
// are in the header.  Both stages move bytes and do a few dozen integer operations per sample: memory-bound.  from_rgb gives each
// thread 4 x 2 pixels -- 24 bytes in (three dword loads per row where the row is aligned), two dword stores of luma and its own
// chroma samples out.  The FDCT reads each sample row with one 8-byte load and the table row with one 16-byte load and stores each
// coefficient row with one 16-byte store; its passes exchange the block through LDS (rows padded to 9 words).
#include "common.h"
#include "jpeg_huff_enc.h"
#include "jpeg_imgs.h"

namespace {

constexpr int kBlocksPerGroup = 32;   // 8 threads per 8 x 8 block, 256 threads
constexpr int kRow = 9, kBlockWords = 8 * kRow + 1;

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }

// four pixels of one row from column x, each as r | g << 8 | b << 16; columns past the image repeat the last one
__device__ __forceinline__ void load_rgb4(const uint8_t* __restrict__ row, int x, int W, uint32_t (&px)[4]) {
  const uint8_t* p = row + (size_t)x * 3;
  if (x + 4 <= W && ((uintptr_t)p & 3) == 0) {
    const uint32_t w0 = reinterpret_cast<const uint32_t*>(p)[0], w1 = reinterpret_cast<const uint32_t*>(p)[1],
                   w2 = reinterpret_cast<const uint32_t*>(p)[2];
    px[0] = w0 & 0xFFFFFFu;
    px[1] = (w0 >> 24) | ((w1 & 0xFFFFu) << 8);
    px[2] = (w1 >> 16) | ((w2 & 0xFFu) << 16);
    px[3] = w2 >> 8;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint8_t* q = row + (size_t)min(x + i, W - 1) * 3;
      px[i] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
    }
  }
}

// jccolor.c's fixed-point tables
__device__ __forceinline__ int luma_of(uint32_t p) {
  const int r = p & 0xFF, g = (p >> 8) & 0xFF, b = (p >> 16) & 0xFF;
  return (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16;
}
__device__ __forceinline__ void chroma_of(uint32_t p, int& cb, int& cr) {
  const int r = p & 0xFF, g = (p >> 8) & 0xFF, b = (p >> 16) & 0xFF;
  cb = (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16;
  cr = (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
}

__device__ __forceinline__ uint32_t pack4(const int (&v)[4]) {
  return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16) | ((uint32_t)v[3] << 24);
}

// one thread: luma columns x .. x + 3 of rows y, y + 1 of the (MCU-padded) planes of image blockIdx.z, and the chroma samples
// that lie under them
__global__ __launch_bounds__(256) void jpeg_from_rgb_kernel(const uint8_t* __restrict__ frames, int Hmax, int Wmax, int channels,
                                                            const vunet_jpeg_img* __restrict__ imgs, uint8_t* __restrict__ planes) {
  const vunet_jpeg_img im = imgs[blockIdx.z];
  const int x = (blockIdx.x * blockDim.x + threadIdx.x) * 4, y = blockIdx.y * 2;
  const int PW = im.bw0 * 8, PH = im.bh0 * 8, W = im.width, H = im.height;
  if (x >= PW || y >= PH) return;
  const size_t pitch = (size_t)Wmax * channels;
  const uint8_t* src = frames + (size_t)im.slot * Hmax * pitch;
  uint8_t* p0 = planes + (size_t)im.plane_off;
  const int ly[2] = {min(y, H - 1), min(y + 1, H - 1)};
  if (channels == 1) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const uint8_t* row = src + (size_t)ly[r] * pitch;
      int v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = row[min(x + i, W - 1)];
      *reinterpret_cast<uint32_t*>(p0 + (size_t)(y + r) * PW + x) = pack4(v);
    }
    return;
  }
  uint32_t px[2][4];
  int cb[2][4], cr[2][4];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    load_rgb4(src + (size_t)ly[r] * pitch, x, W, px[r]);
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = luma_of(px[r][i]);
    *reinterpret_cast<uint32_t*>(p0 + (size_t)(y + r) * PW + x) = pack4(v);
  }
  const int CW = im.bw1 * 8, CH = im.bh1 * 8;
  uint8_t* p1 = p0 + (size_t)PW * PH;
  uint8_t* p2 = p1 + (size_t)CW * CH;
  if (im.vsamp == 2) {
    // the chroma row under these two luma rows; below the last down-sampled row THAT row is repeated, not the last image row
    const int jj = min(y >> 1, ((H + 1) >> 1) - 1);
    const int c0 = min(2 * jj, H - 1), c1 = min(2 * jj + 1, H - 1);
    if (c0 != ly[0] || c1 != ly[1]) {
      load_rgb4(src + (size_t)c0 * pitch, x, W, px[0]);
      load_rgb4(src + (size_t)c1 * pitch, x, W, px[1]);
    }
  }
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int i = 0; i < 4; ++i) chroma_of(px[r][i], cb[r][i], cr[r][i]);
  if (im.hsamp == 1) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      *reinterpret_cast<uint32_t*>(p1 + (size_t)(y + r) * CW + x) = pack4(cb[r]);
      *reinterpret_cast<uint32_t*>(p2 + (size_t)(y + r) * CW + x) = pack4(cr[r]);
    }
  } else if (im.vsamp == 1) {   // h2v1: bias 0, 1, 0, 1, .. along the output columns (x / 2 is even)
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const size_t at = (size_t)(y + r) * CW + (x >> 1);
      *reinterpret_cast<uint16_t*>(p1 + at) = (uint16_t)(((cb[r][0] + cb[r][1]) >> 1) | (((cb[r][2] + cb[r][3] + 1) >> 1) << 8));
      *reinterpret_cast<uint16_t*>(p2 + at) = (uint16_t)(((cr[r][0] + cr[r][1]) >> 1) | (((cr[r][2] + cr[r][3] + 1) >> 1) << 8));
    }
  } else {                      // h2v2: bias 1, 2, 1, 2, ..
    const size_t at = (size_t)(y >> 1) * CW + (x >> 1);
    *reinterpret_cast<uint16_t*>(p1 + at) = (uint16_t)(((cb[0][0] + cb[0][1] + cb[1][0] + cb[1][1] + 1) >> 2) |
                                                       (((cb[0][2] + cb[0][3] + cb[1][2] + cb[1][3] + 2) >> 2) << 8));
    *reinterpret_cast<uint16_t*>(p2 + at) = (uint16_t)(((cr[0][0] + cr[0][1] + cr[1][0] + cr[1][1] + 1) >> 2) |
                                                       (((cr[0][2] + cr[0][3] + cr[1][2] + cr[1][3] + 2) >> 2) << 8));
  }
}

// jfdctint.c, one 1-D pass: CONST_BITS 13, PASS1_BITS 2.  FIRST: the row pass (outputs 0 and 4 scaled up by 2 bits, the others
// descaled by 11); otherwise the column pass (0 and 4 descaled by 2, the others by 15).  32-bit integers suffice for 8-bit samples
template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int32_t (&d)[8], int32_t (&out)[8]) {
  constexpr int32_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                    F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  constexpr int N = FIRST ? 11 : 15;
  constexpr int32_t half = 1 << (N - 1);
  const int32_t tmp0 = d[0] + d[7], tmp1 = d[1] + d[6], tmp2 = d[2] + d[5], tmp3 = d[3] + d[4];
  int32_t tmp7 = d[0] - d[7], tmp6 = d[1] - d[6], tmp5 = d[2] - d[5], tmp4 = d[3] - d[4];
  const int32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  if (FIRST) {
    out[0] = (tmp10 + tmp11) * 4;
    out[4] = (tmp10 - tmp11) * 4;
  } else {
    out[0] = (tmp10 + tmp11 + 2) >> 2;
    out[4] = (tmp10 - tmp11 + 2) >> 2;
  }
  int32_t z1 = (tmp12 + tmp13) * F0_541;
  out[2] = (z1 + tmp13 * F0_765 + half) >> N;
  out[6] = (z1 + tmp12 * (-F1_847) + half) >> N;
  z1 = tmp4 + tmp7;
  int32_t z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
  const int32_t z5 = (z3 + z4) * F1_175;
  tmp4 *= F0_298;
  tmp5 *= F2_053;
  tmp6 *= F3_072;
  tmp7 *= F1_501;
  z1 *= -F0_899;
  z2 *= -F2_562;
  z3 *= -F1_961;
  z4 *= -F0_390;
  z3 += z5;
  z4 += z5;
  out[7] = (tmp4 + z1 + z3 + half) >> N;
  out[5] = (tmp5 + z2 + z4 + half) >> N;
  out[3] = (tmp6 + z2 + z3 + half) >> N;
  out[1] = (tmp7 + z1 + z4 + half) >> N;
}

__global__ __launch_bounds__(256) void jpeg_fdct_kernel(const uint8_t* __restrict__ planes, const uint16_t* __restrict__ qtab,
                                                        const vunet_jpeg_img* __restrict__ imgs, int N, int total,
                                                        int16_t* __restrict__ coef) {
  __shared__ int32_t ws[kBlocksPerGroup * kBlockWords];   // jfdctint.c's in-place block, one per 8 x 8 block
  const int b = threadIdx.x >> 3, t = threadIdx.x & 7;
  const int g = blockIdx.x * kBlocksPerGroup + b;
  const bool live = g < total;
  int32_t* w = ws + b * kBlockWords;
  int16_t* dst = nullptr;
  const uint16_t* q = nullptr;
  bool dummy = false;
  if (live) {
    int lo = 0, hi = N - 1;                       // the last image whose first block is <= g
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (imgs[mid].block0 <= g) lo = mid; else hi = mid - 1;
    }
    const vunet_jpeg_img im = imgs[lo];
    const int l = g - im.block0, n0 = im.bw0 * im.bh0, n1 = im.bw1 * im.bh1;
    int c = 0, idx = l, bw = im.bw0, hsc = im.hsamp;
    int ew = im.width, eh = im.height;            // the component's real extent in samples
    size_t plane = (size_t)im.plane_off;
    if (l >= n0) {
      c = 1 + (l - n0) / n1;
      idx = (l - n0) % n1;
      bw = im.bw1;
      hsc = 1;
      ew = (im.width + im.hsamp - 1) / im.hsamp;
      eh = (im.height + im.vsamp - 1) / im.vsamp;
      plane += (size_t)n0 * 64 + (size_t)(c - 1) * n1 * 64;
    }
    const int wb = (ew + 7) >> 3, hb = (eh + 7) >> 3;
    int brow = idx / bw, bcol = idx % bw;
    // a dummy block (MCU padding) repeats the DC of a real one: these eight threads transform THAT block and keep its DC
    if (brow >= hb) {
      dummy = true;
      brow = hb - 1;
      bcol = min((bcol / hsc) * hsc + hsc - 1, wb - 1);
    } else if (bcol >= wb) {
      dummy = true;
      bcol = wb - 1;
    }
    dst = coef + (size_t)im.coef_off + (size_t)l * 64 + t * 8;
    q = qtab + (size_t)im.q_off + (size_t)c * 64 + t * 8;
    // row t of the block: eight samples, one 8-byte load; level shift; the row pass
    const uint2 sv = *reinterpret_cast<const uint2*>(planes + plane + ((size_t)brow * 8 + t) * ((size_t)bw * 8) + (size_t)bcol * 8);
    int32_t in[8], out[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      in[j] = (int32_t)((sv.x >> (8 * j)) & 0xFF) - 128;
      in[4 + j] = (int32_t)((sv.y >> (8 * j)) & 0xFF) - 128;
    }
    fdct_1d<true>(in, out);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[t * kRow + j] = out[j];
  }
  __syncthreads();
  if (live) {   // column t
    int32_t in[8], out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = w[r * kRow + t];
    fdct_1d<false>(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * kRow + t] = out[r];
  }
  __syncthreads();
  if (live) {   // row t of the coefficients: quantise, one 16-byte store
    const uint4 qv = *reinterpret_cast<const uint4*>(q);
    const uint32_t qw[4] = {qv.x, qv.y, qv.z, qv.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t pair = 0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int32_t v = w[t * kRow + 2 * j + k];
        const uint32_t d = ((qw[j] >> (16 * k)) & 0xFFFF) * 8;
        const uint32_t m = ((uint32_t)(v < 0 ? -v : v) + (d >> 1)) / d;
        const int32_t s = v < 0 ? -(int32_t)m : (int32_t)m;
        pair |= ((uint32_t)s & 0xFFFF) << (16 * k);
      }
      o[j] = pair;
    }
    if (dummy) {
      o[0] = t == 0 ? (o[0] & 0xFFFF) : 0;
      o[1] = o[2] = o[3] = 0;
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

}  // namespace

extern "C" int vunet_jpeg_encode_info(int32_t height, int32_t width, int32_t ncomp, int32_t hsamp, int32_t vsamp,
                                      vunet_jpeg_info* info) {
  return vunet_jpeg::encode_info(height, width, ncomp, hsamp, vsamp, info);
}

extern "C" int vunet_jpeg_quant_tables(int32_t quality, uint16_t* qtab) { return vunet_jpeg::quant_tables(quality, qtab); }

extern "C" int vunet_jpeg_encode_bound(const vunet_jpeg_info* info, int64_t* bytes) { return vunet_jpeg::encode_bound(info, bytes); }

extern "C" int vunet_jpeg_entropy_encode(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, uint8_t* out,
                                         int64_t cap, int64_t* len) {
  return vunet_jpeg::entropy_encode(coef, info, qtab, out, cap, len);
}

extern "C" int vunet_jpeg_symbol_histogram(const int16_t* coef, const vunet_jpeg_info* info, uint32_t* hist) {
  return vunet_jpeg::symbol_histogram(coef, info, hist);
}

extern "C" int vunet_jpeg_optimal_table(const uint32_t* freq, uint8_t* counts, uint8_t* symbols, int32_t* nsym) {
  return vunet_jpeg::optimal_table(freq, counts, symbols, nsym);
}

extern "C" int vunet_jpeg_optimal_tables(const uint32_t* hist, int32_t N, int32_t ntab, uint8_t* counts, uint8_t* symbols,
                                         uint32_t* codes, int32_t* failed) {
  return vunet_jpeg::optimal_tables(hist, N, ntab, counts, symbols, codes, failed);
}

extern "C" int vunet_jpeg_entropy_encode_tables(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab,
                                                const uint8_t* counts, const uint8_t* symbols, uint8_t* out, int64_t cap,
                                                int64_t* len) {
  return vunet_jpeg::entropy_encode_tables(coef, info, qtab, counts, symbols, out, cap, len);
}

extern "C" int vunet_jpeg_write_header(const vunet_jpeg_info* info, const uint16_t* qtab, const uint8_t* counts,
                                       const uint8_t* symbols, uint8_t* out, int64_t cap, int64_t* len) {
  return vunet_jpeg::write_header(info, qtab, counts, symbols, out, cap, len);
}

extern "C" int vunet_jpeg_code_words(const uint8_t* counts, const uint8_t* symbols, uint32_t* codes) {
  if (!codes || !counts != !symbols) return VUNET_ERR_ARG;
  vunet_jpeg::Tables t = vunet_jpeg::std_tables();
  if (counts && !vunet_jpeg::caller_tables(counts, symbols, 4, t)) return VUNET_ERR_ARG;
  vunet_jpeg::code_words(t, 4, codes);
  return VUNET_OK;
}

extern "C" int vunet_jpeg_from_rgb(const uint8_t* frames, int32_t Nslots, int32_t Hmax, int32_t Wmax, int32_t channels,
                                   const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, uint8_t* planes,
                                   int64_t planes_bytes, void* stream) {
  int64_t total = 0;
  if (!frames || !imgs || !imgs_host || !planes || N < 1 || N > 65535 || Nslots < 1 || Nslots > 65535 || Hmax < 1 || Hmax > 65535 ||
      Wmax < 1 || Wmax > 65535 || (channels != 1 && channels != 3) || planes_bytes < 0 || !vunet_jpeg::aligned16(planes) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, INT64_MAX, INT64_MAX, planes_bytes, Hmax, Wmax, Nslots, &total) ||
      !vunet_jpeg::grids_exact(imgs_host, N, channels))
    return VUNET_ERR_ARG;
  int pw = 0, ph = 0;   // the largest padded luma plane: what the grid has to cover
  for (int n = 0; n < N; ++n) {
    pw = imgs_host[n].bw0 * 8 > pw ? imgs_host[n].bw0 * 8 : pw;
    ph = imgs_host[n].bh0 * 8 > ph ? imgs_host[n].bh0 * 8 : ph;
  }
  const int quads = pw / 4;
  const unsigned lanes = quads >= 256 ? 256u : (unsigned)((quads + 63) / 64 * 64);
  VUNET_LAUNCH(jpeg_from_rgb_kernel, dim3((unsigned)((quads + (int)lanes - 1) / (int)lanes), (unsigned)(ph / 2), (unsigned)N),
               dim3(lanes), 0, (hipStream_t)stream, frames, (int)Hmax, (int)Wmax, (int)channels, imgs, planes);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_fdct(const uint8_t* planes, int64_t planes_bytes, const uint16_t* qtab, int64_t qtab_count,
                               const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, int16_t* coef,
                               int64_t coef_count, void* stream) {
  int64_t total = 0;
  if (!planes || !qtab || !imgs || !imgs_host || !coef || N < 1 || N > 65535 || coef_count < 0 || qtab_count < 0 || planes_bytes < 0 ||
      !vunet_jpeg::aligned16(coef) || !vunet_jpeg::aligned16(qtab) || !vunet_jpeg::aligned16(planes) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, coef_count, qtab_count, planes_bytes, 65535, 65535, 65535, &total) ||
      !vunet_jpeg::grids_exact(imgs_host, N, 0))
    return VUNET_ERR_ARG;
  const unsigned groups = (unsigned)((total + kBlocksPerGroup - 1) / kBlocksPerGroup);
  VUNET_LAUNCH(jpeg_fdct_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, planes, qtab, imgs, (int)N, (int)total, coef);
  return vunet_check_launch();
}
