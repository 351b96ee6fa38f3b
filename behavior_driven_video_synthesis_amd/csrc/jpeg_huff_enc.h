// The host half of the baseline JPEG encoder: the quantisation tables, the stream's segments and the Huffman coder.  Plain C++17,
// no HIP, header-only; included by jpeg_enc.hip (the C ABI of include/vunet_jpeg_enc.h) and by tools/jpeg_enc_host_check.cpp.  The
// mirror image of jpeg_entropy.h, whose coefficient layout and zigzag table it shares.  Every byte goes through Sink::put, which
// counts it always and stores it only below `cap` (put_bits stores four at once where all four fit, and falls back to put where
// they do not): nothing is written at or beyond out + cap, and the count at the end is the length the stream needs.
// Errors are VUNET_ERR_ARG and VUNET_JPEG_ERR_CAPACITY / _RANGE; nothing throws, nothing is static but the constant tables.
//
// The Huffman tables are Annex K's (libjpeg's defaults, std_huff_tables); no optimised tables, no restart markers.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/vunet_jpeg_enc.h"
#include "jpeg_entropy.h"

namespace vunet_jpeg {

// Annex K.1, natural order
static const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                      69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                      81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
static const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                        99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// Annex K.3: code counts per length 1 .. 16, then the symbols
static const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

constexpr int64_t kHeaderBound = 1024;    // SOI .. SOS and EOI: 623 bytes with three components
constexpr int64_t kBlockBound = 416;      // 22 bits of DC + 63 * 26 bits of AC = 208 bytes, every one of them stuffed

inline int encode_info(int32_t height, int32_t width, int32_t ncomp, int32_t hs, int32_t vs, vunet_jpeg_info* info) {
  if (!info || height < 1 || width < 1 || height > 65535 || width > 65535) return VUNET_ERR_ARG;
  const bool s = (hs == 1 && vs == 1) || (ncomp == 3 && hs == 2 && (vs == 1 || vs == 2));
  if (!s || (ncomp != 1 && ncomp != 3)) return VUNET_ERR_ARG;
  vunet_jpeg_info& I = *info;
  I.height = height;
  I.width = width;
  I.ncomp = ncomp;
  I.hsamp = hs;
  I.vsamp = vs;
  I.mcu_cols = (width + 8 * hs - 1) / (8 * hs);
  I.mcu_rows = (height + 8 * vs - 1) / (8 * vs);
  I.restart = 0;
  I.bw0 = I.mcu_cols * hs;
  I.bh0 = I.mcu_rows * vs;
  I.bw1 = ncomp == 3 ? I.mcu_cols : 0;
  I.bh1 = ncomp == 3 ? I.mcu_rows : 0;
  const int64_t nblocks = (int64_t)I.bw0 * I.bh0 + 2 * (int64_t)I.bw1 * I.bh1;
  if (nblocks > (0x7FFFFFFF >> 6)) return VUNET_ERR_ARG;
  I.nblocks = (int32_t)nblocks;
  I.ncoef = I.nblocks * 64;
  return VUNET_OK;
}

// the info is one encode_info gives (so every size below follows from five checked numbers)
inline bool encode_info_ok(const vunet_jpeg_info& I) {
  vunet_jpeg_info want;
  return encode_info(I.height, I.width, I.ncomp, I.hsamp, I.vsamp, &want) == VUNET_OK && same_info(I, want);
}

inline int quant_tables(int32_t quality, uint16_t* qtab) {
  if (!qtab) return VUNET_ERR_ARG;
  const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
  const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = ((t ? kBaseChroma[i] : kBaseLuma[i]) * scale + 50) / 100;
      qtab[64 * t + i] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  return VUNET_OK;
}

inline int encode_bound(const vunet_jpeg_info* info, int64_t* bytes) {
  if (!info || !bytes || !encode_info_ok(*info)) return VUNET_ERR_ARG;
  *bytes = kHeaderBound + kBlockBound * (int64_t)info->nblocks;
  return VUNET_OK;
}

struct Sink {
  uint8_t* out;
  int64_t cap, n = 0;
  uint64_t acc = 0;   // the low `bits` bits are waiting
  int bits = 0;

  inline void put(int b) {
    if (n < cap) out[n] = (uint8_t)b;
    ++n;
  }
  inline void put16(int v) {
    put(v >> 8);
    put(v & 0xFF);
  }
  inline void put_bytes(const uint8_t* p, int count) {
    for (int i = 0; i < count; ++i) put(p[i]);
  }
  inline void put_stuffed(int b) {
    put(b);
    if (b == 0xFF) put(0);   // a zero byte after every 0xFF of the scan
  }
  // `len` <= 26 bits of `code` (no bits above them set); at most 31 wait between calls.  Four bytes leave at a time: in one store
  // where none of them is 0xFF and all four fit, one by one otherwise
  inline void put_bits(uint32_t code, int len) {
    acc = (acc << len) | code;
    bits += len;
    if (bits >= 32) {
      bits -= 32;
      const uint32_t w = (uint32_t)(acc >> bits);
      if (n + 4 <= cap && ((~w - 0x01010101u) & w & 0x80808080u) == 0) {
        out[n] = (uint8_t)(w >> 24);
        out[n + 1] = (uint8_t)(w >> 16);
        out[n + 2] = (uint8_t)(w >> 8);
        out[n + 3] = (uint8_t)w;
        n += 4;
      } else {
        for (int s = 24; s >= 0; s -= 8) put_stuffed((int)((w >> s) & 0xFF));
      }
    }
  }
  // the whole bytes that wait, then the last one padded with 1-bits
  inline void flush_bits() {
    while (bits >= 8) {
      bits -= 8;
      put_stuffed((int)((acc >> bits) & 0xFF));
    }
    if (bits) put_stuffed((int)(((acc << (8 - bits)) | ((1u << (8 - bits)) - 1)) & 0xFF));
    acc = 0;
    bits = 0;
  }
};

struct Codes {
  uint16_t code[256];
  uint8_t len[256];   // 0: no such symbol
};

inline void build_codes(const uint8_t* counts, const uint8_t* symbols, Codes& c) {
  memset(&c, 0, sizeof(c));
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
      c.code[symbols[k]] = (uint16_t)code;
      c.len[symbols[k]] = (uint8_t)len;
    }
    code <<= 1;
  }
}

inline void put_dht(Sink& s, int cls_id, const uint8_t* counts, const uint8_t* symbols, int total) {
  s.put16(0xFFC4);
  s.put16(2 + 1 + 16 + total);
  s.put(cls_id);
  s.put_bytes(counts, 16);
  s.put_bytes(symbols, total);
}

inline int bit_length(uint32_t v) { return v ? 32 - __builtin_clz(v) : 0; }

inline int entropy_encode(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, uint8_t* out, int64_t cap,
                          int64_t* len) {
  if (!coef || !info || !qtab || !out || !len || cap < 0 || !encode_info_ok(*info)) return VUNET_ERR_ARG;
  *len = 0;
  const vunet_jpeg_info& I = *info;
  for (int i = 0; i < 64 * I.ncomp; ++i)
    if (qtab[i] < 1 || qtab[i] > 255) return VUNET_ERR_ARG;
  if (I.ncomp == 3 && memcmp(qtab + 64, qtab + 128, 64 * sizeof(uint16_t)) != 0) return VUNET_ERR_ARG;
  const int ntab = I.ncomp == 3 ? 2 : 1;
  Sink s{out, cap};
  s.put16(0xFFD8);
  static const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  s.put_bytes(app0, 18);
  for (int t = 0; t < ntab; ++t) {
    s.put16(0xFFDB);
    s.put16(67);
    s.put(t);
    for (int i = 0; i < 64; ++i) s.put(qtab[64 * t + kZigzag[i]]);
  }
  s.put16(0xFFC0);
  s.put16(8 + 3 * I.ncomp);
  s.put(8);
  s.put16(I.height);
  s.put16(I.width);
  s.put(I.ncomp);
  for (int c = 0; c < I.ncomp; ++c) {
    s.put(c + 1);
    s.put(c == 0 ? (I.hsamp << 4 | I.vsamp) : 0x11);
    s.put(c == 0 ? 0 : 1);
  }
  put_dht(s, 0x00, kDcLumaBits, kDcVals, 12);
  put_dht(s, 0x10, kAcLumaBits, kAcLumaVals, 162);
  if (I.ncomp == 3) {
    put_dht(s, 0x01, kDcChromaBits, kDcVals, 12);
    put_dht(s, 0x11, kAcChromaBits, kAcChromaVals, 162);
  }
  s.put16(0xFFDA);
  s.put16(6 + 2 * I.ncomp);
  s.put(I.ncomp);
  for (int c = 0; c < I.ncomp; ++c) {
    s.put(c + 1);
    s.put(c == 0 ? 0x00 : 0x11);
  }
  s.put(0);
  s.put(63);
  s.put(0);

  Codes dc[2], ac[2];
  build_codes(kDcLumaBits, kDcVals, dc[0]);
  build_codes(kAcLumaBits, kAcLumaVals, ac[0]);
  build_codes(kDcChromaBits, kDcVals, dc[1]);
  build_codes(kAcChromaBits, kAcChromaVals, ac[1]);
  const int16_t* base[3];
  int bw[3], nh[3], nv[3];
  base[0] = coef;
  bw[0] = I.bw0;
  nh[0] = I.hsamp;
  nv[0] = I.vsamp;
  for (int c = 1; c < I.ncomp; ++c) {
    base[c] = coef + 64 * ((int64_t)I.bw0 * I.bh0 + (int64_t)(c - 1) * I.bw1 * I.bh1);
    bw[c] = I.bw1;
    nh[c] = nv[c] = 1;
  }
  int32_t pred[3] = {0, 0, 0};
  for (int my = 0; my < I.mcu_rows; ++my) {
    for (int mx = 0; mx < I.mcu_cols; ++mx) {
      for (int c = 0; c < I.ncomp; ++c) {
        const Codes& hd = dc[c ? 1 : 0];
        const Codes& ha = ac[c ? 1 : 0];
        for (int by = 0; by < nv[c]; ++by) {
          for (int bx = 0; bx < nh[c]; ++bx) {
            const int16_t* blk = base[c] + 64 * ((int64_t)(my * nv[c] + by) * bw[c] + (mx * nh[c] + bx));
            const int32_t diff = (int32_t)blk[0] - pred[c];
            pred[c] = blk[0];
            int nb = bit_length((uint32_t)(diff < 0 ? -diff : diff));
            if (nb > 11) return VUNET_JPEG_ERR_RANGE;
            s.put_bits(hd.code[nb], hd.len[nb]);
            if (nb) s.put_bits((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
            int run = 0;
            for (int k = 1; k < 64; ++k) {
              const int32_t v = blk[kZigzag[k]];
              if (v == 0) {
                ++run;
                continue;
              }
              for (; run > 15; run -= 16) s.put_bits(ha.code[0xF0], ha.len[0xF0]);
              nb = bit_length((uint32_t)(v < 0 ? -v : v));
              if (nb > 10) return VUNET_JPEG_ERR_RANGE;
              const int sym = (run << 4) | nb;
              s.put_bits(((uint32_t)ha.code[sym] << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1)), ha.len[sym] + nb);
              run = 0;
            }
            if (run) s.put_bits(ha.code[0x00], ha.len[0x00]);
          }
        }
      }
    }
  }
  s.flush_bits();
  s.put16(0xFFD9);
  *len = s.n;
  return s.n > cap ? VUNET_JPEG_ERR_CAPACITY : VUNET_OK;
}

}  // namespace vunet_jpeg
