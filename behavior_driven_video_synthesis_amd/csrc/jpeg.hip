// Baseline JPEG decode: the C ABI of include/vunet_jpeg.h.  The host half (marker parse, Huffman walk) is jpeg_entropy.h and calls
// no HIP; the device half is here -- dequantisation + libjpeg's integer "islow" inverse DCT, and the chroma up-sampling + YCbCr ->
// RGB conversion into the uint8 stack of the raw-frame route.  Two launches per batch, whatever the images' sizes and samplings:
// one vunet_jpeg_img row per image says where its coefficients, tables and planes lie.
//
// The reference reads every frame with cv2.imread on the host (data/base_dataset.py), i.e. libjpeg-turbo's defaults; the rules
// restated from jidctint.c, jdsample.c and jdcolor.c are in the header.  Both stages move bytes and do a few dozen integer
// operations per sample: memory-bound.  The IDCT reads each coefficient row and table row with one 16-byte load and stores
// each sample row with one 8-byte store; its two passes exchange the block through LDS (rows padded to 9 words).
#include "common.h"
#include "jpeg_entropy.h"
#include "jpeg_imgs.h"

namespace {

constexpr int kBlocksPerGroup = 32;   // 8 threads per 8 x 8 block, 256 threads
constexpr int kRow = 9, kBlockWords = 8 * kRow + 1;

// jidctint.c, one 1-D pass: CONST_BITS 13; `in` dequantised coefficients (pass 1) or the workspace row (pass 2), JLONG = 64-bit
template <int DESCALE>
__device__ __forceinline__ void idct_1d(const int32_t (&in)[8], int64_t (&out)[8]) {
  constexpr int64_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                    F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  int64_t z2 = in[2], z3 = in[6];
  int64_t z1 = (z2 + z3) * F0_541;
  int64_t tmp2 = z1 + z3 * (-F1_847);
  int64_t tmp3 = z1 + z2 * F0_765;
  z2 = in[0];
  z3 = in[4];
  int64_t tmp0 = (z2 + z3) * (1 << 13);
  int64_t tmp1 = (z2 - z3) * (1 << 13);
  const int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = in[7];
  tmp1 = in[5];
  tmp2 = in[3];
  tmp3 = in[1];
  z1 = tmp0 + tmp3;
  z2 = tmp1 + tmp2;
  z3 = tmp0 + tmp2;
  int64_t z4 = tmp1 + tmp3;
  const int64_t z5 = (z3 + z4) * F1_175;
  tmp0 *= F0_298;
  tmp1 *= F2_053;
  tmp2 *= F3_072;
  tmp3 *= F1_501;
  z1 *= -F0_899;
  z2 *= -F2_562;
  z3 *= -F1_961;
  z4 *= -F0_390;
  z3 += z5;
  z4 += z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  constexpr int64_t half = (int64_t)1 << (DESCALE - 1);
  out[0] = (tmp10 + tmp3 + half) >> DESCALE;
  out[7] = (tmp10 - tmp3 + half) >> DESCALE;
  out[1] = (tmp11 + tmp2 + half) >> DESCALE;
  out[6] = (tmp11 - tmp2 + half) >> DESCALE;
  out[2] = (tmp12 + tmp1 + half) >> DESCALE;
  out[5] = (tmp12 - tmp1 + half) >> DESCALE;
  out[3] = (tmp13 + tmp0 + half) >> DESCALE;
  out[4] = (tmp13 - tmp0 + half) >> DESCALE;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint16_t* __restrict__ qtab,
                                                        const vunet_jpeg_img* __restrict__ imgs, int N, int total,
                                                        uint8_t* __restrict__ planes) {
  __shared__ int32_t ws[kBlocksPerGroup * kBlockWords];   // jidctint.c's `int workspace[64]`, one per block
  const int b = threadIdx.x >> 3, t = threadIdx.x & 7;
  const int g = blockIdx.x * kBlocksPerGroup + b;
  const bool live = g < total;
  int32_t* w = ws + b * kBlockWords;
  uint8_t* dst = nullptr;
  if (live) {
    int lo = 0, hi = N - 1;                       // the last image whose first block is <= g
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (imgs[mid].block0 <= g) lo = mid; else hi = mid - 1;
    }
    const vunet_jpeg_img im = imgs[lo];
    const int l = g - im.block0, n0 = im.bw0 * im.bh0, n1 = im.bw1 * im.bh1;
    int c = 0, idx = l, bw = im.bw0;
    size_t plane = (size_t)im.plane_off;
    if (l >= n0) {
      c = 1 + (l - n0) / n1;
      idx = (l - n0) % n1;
      bw = im.bw1;
      plane += (size_t)n0 * 64 + (size_t)(c - 1) * n1 * 64;
    }
    const int brow = idx / bw, bcol = idx % bw;
    dst = planes + plane + ((size_t)brow * 8 + t) * ((size_t)bw * 8) + (size_t)bcol * 8;
    // row t of the block and of its table: eight int16 / uint16 each, one 16-byte load each
    const uint4 cv = *reinterpret_cast<const uint4*>(coef + (size_t)im.coef_off + (size_t)l * 64 + t * 8);
    const uint4 qv = *reinterpret_cast<const uint4*>(qtab + (size_t)im.q_off + (size_t)c * 64 + t * 8);
    const uint32_t cw[4] = {cv.x, cv.y, cv.z, cv.w}, qw[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      w[t * kRow + 2 * j] = (int32_t)(int16_t)(cw[j] & 0xFFFF) * (int32_t)(qw[j] & 0xFFFF);
      w[t * kRow + 2 * j + 1] = (int32_t)(int16_t)(cw[j] >> 16) * (int32_t)(qw[j] >> 16);
    }
  }
  __syncthreads();
  if (live) {   // pass 1: column t
    int32_t in[8];
    int64_t out[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) in[r] = w[r * kRow + t];
    idct_1d<13 - 2>(in, out);
#pragma unroll
    for (int r = 0; r < 8; ++r) w[r * kRow + t] = (int32_t)out[r];
  }
  __syncthreads();
  if (live) {   // pass 2: row t, + 128, clamp
    int32_t in[8];
    int64_t out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) in[j] = w[t * kRow + j];
    idct_1d<13 + 2 + 3>(in, out);
    uint32_t px[2] = {0, 0};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t v = out[j] + 128;
      const uint32_t s = (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
      px[j >> 2] |= s << (8 * (j & 3));
    }
    *reinterpret_cast<uint2*>(dst) = make_uint2(px[0], px[1]);
  }
}

// one up-sampled chroma sample (jdsample.c: h2v1 / h2v2 "fancy" filters where the down-sampled width is more than 2, replication
// below that), on the real down-sampled extent cw x ch with the edges replicated
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ p, size_t stride, int x, int y, int hs, int vs, int cw, int ch) {
  if (hs == 1) return p[(size_t)y * stride + x];
  const int i = x >> 1;
  if (cw <= 2) return p[(size_t)(vs == 2 ? y >> 1 : y) * stride + i];
  if (vs == 1) {
    const uint8_t* row = p + (size_t)y * stride;
    const int cur = row[i];
    if (x & 1) return i == cw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
    return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
  }
  const int j = y >> 1;
  const uint8_t* near = p + (size_t)j * stride;
  const uint8_t* far = p + (size_t)((y & 1) ? min(j + 1, ch - 1) : max(j - 1, 0)) * stride;
  const int s = 3 * near[i] + far[i];
  if (x & 1) return i == cw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
  return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ uint8_t clamp255(int v) { return (uint8_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void jpeg_to_rgb_kernel(const uint8_t* __restrict__ planes, const vunet_jpeg_img* __restrict__ imgs,
                                                          int Hmax, int Wmax, uint8_t* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  const vunet_jpeg_img im = imgs[n];
  if (x >= im.width || y >= im.height) return;   // (bytes outside the image are not touched)
  const uint8_t* p0 = planes + (size_t)im.plane_off;
  const size_t s0 = (size_t)im.bw0 * 8;
  const int Y = p0[(size_t)y * s0 + x];
  int r = Y, g = Y, b = Y;
  if (im.ncomp == 3) {
    const size_t s1 = (size_t)im.bw1 * 8, n1 = s1 * (size_t)im.bh1 * 8;
    const uint8_t* p1 = p0 + s0 * (size_t)im.bh0 * 8;
    const int cw = (im.width + im.hsamp - 1) / im.hsamp, ch = (im.height + im.vsamp - 1) / im.vsamp;
    const int cb = chroma_at(p1, s1, x, y, im.hsamp, im.vsamp, cw, ch) - 128;
    const int cr = chroma_at(p1 + n1, s1, x, y, im.hsamp, im.vsamp, cw, ch) - 128;
    r = Y + ((91881 * cr + 32768) >> 16);
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    b = Y + ((116130 * cb + 32768) >> 16);
  }
  uint8_t* o = out + (((size_t)im.slot * Hmax + y) * Wmax + x) * 3;
  o[0] = clamp255(r);
  o[1] = clamp255(g);
  o[2] = clamp255(b);
}

}  // namespace

extern "C" int vunet_jpeg_parse(const uint8_t* bytes, int64_t len, vunet_jpeg_info* info) {
  return vunet_jpeg::parse_info(bytes, len, info);
}

extern "C" int vunet_jpeg_entropy_decode(const uint8_t* bytes, int64_t len, const vunet_jpeg_info* info, int16_t* coef,
                                         uint16_t* qtab) {
  return vunet_jpeg::entropy_decode(bytes, len, info, coef, qtab);
}

extern "C" int vunet_jpeg_idct(const int16_t* coef, int64_t coef_count, const uint16_t* qtab, int64_t qtab_count,
                               const vunet_jpeg_img* imgs, const vunet_jpeg_img* imgs_host, int32_t N, uint8_t* planes,
                               int64_t planes_bytes, void* stream) {
  int64_t total = 0;
  if (!coef || !qtab || !imgs || !imgs_host || !planes || N < 1 || N > 65535 || coef_count < 0 || qtab_count < 0 || planes_bytes < 0 ||
      !vunet_jpeg::aligned16(coef) || !vunet_jpeg::aligned16(qtab) || !vunet_jpeg::aligned16(planes) ||
      !vunet_jpeg::imgs_ok(imgs_host, N, coef_count, qtab_count, planes_bytes, 65535, 65535, 65535, &total))
    return VUNET_ERR_ARG;
  const unsigned groups = (unsigned)((total + kBlocksPerGroup - 1) / kBlocksPerGroup);
  VUNET_LAUNCH(jpeg_idct_kernel, dim3(groups), dim3(256), 0, (hipStream_t)stream, coef, qtab, imgs, (int)N, (int)total, planes);
  return vunet_check_launch();
}

extern "C" int vunet_jpeg_to_rgb(const uint8_t* planes, int64_t planes_bytes, const vunet_jpeg_img* imgs,
                                 const vunet_jpeg_img* imgs_host, int32_t N, int32_t Nslots, int32_t Hmax, int32_t Wmax, uint8_t* out,
                                 void* stream) {
  int64_t total = 0;
  if (!planes || !imgs || !imgs_host || !out || N < 1 || N > 65535 || Nslots < N || Nslots > 65535 || Hmax < 1 || Hmax > 65535 || Wmax < 1 || Wmax > 65535 ||
      planes_bytes < 0 || !vunet_jpeg::imgs_ok(imgs_host, N, INT64_MAX, INT64_MAX, planes_bytes, Hmax, Wmax, Nslots, &total))
    return VUNET_ERR_ARG;
  const unsigned lanes = Wmax >= 256 ? 256u : (unsigned)((Wmax + 63) / 64 * 64);
  VUNET_LAUNCH(jpeg_to_rgb_kernel, dim3((unsigned)((Wmax + (int)lanes - 1) / (int)lanes), (unsigned)Hmax, (unsigned)N), dim3(lanes), 0,
               (hipStream_t)stream, planes, imgs, (int)Hmax, (int)Wmax, out);
  return vunet_check_launch();
}
