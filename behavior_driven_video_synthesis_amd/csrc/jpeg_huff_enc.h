// The host half of the baseline JPEG encoder: the quantisation tables, the stream's segments and the Huffman coder.  Plain C++17,
// no HIP, header-only; included by jpeg_enc.hip (the C ABI of include/vunet_jpeg_enc.h), by jpeg_huff.hip (the same coder as device
// launches; its argument checks are here) and by tools/jpeg_enc_host_check.cpp and tools/jpeg_opt_host_check.cpp.  The
// mirror image of jpeg_entropy.h, whose coefficient layout and zigzag table it shares.  Every byte goes through Sink::put, which
// counts it always and stores it only below `cap` (put_bits stores four at once where all four fit, and falls back to put where
// they do not): nothing is written at or beyond out + cap, and the count at the end is the length the stream needs.
// Errors are VUNET_ERR_ARG and VUNET_JPEG_ERR_CAPACITY / _RANGE; nothing throws, nothing is static but the constant tables.
//
// The Huffman tables are Annex K's (libjpeg's defaults, std_huff_tables) or the caller's; symbol_histogram and optimal_table give
// the tables libjpeg's optimize_coding (Pillow's optimize=True) would: a second pass over the coefficients.  code_words states
// tables as the device coder (jpeg_huff.hip) reads them, write_header writes SOI .. SOS alone for it.  No restart markers.
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
constexpr int64_t kBlockBits = 27 + 63 * 26;   // under any tables: a 16-bit code and 11 bits of DC, 16 and 10 per AC term
constexpr int64_t kStuffChunk = 1024;     // the device coder's unstuffed streams start at multiples of it (jpeg_huff.hip)

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

// the block grids of every descriptor row are exactly what encode_info gives (the kernels' padding, dummy-block and scan-order
// rules assume it); ncomp != 0: and every row has that many components
inline bool grids_exact(const vunet_jpeg_img* h, int N, int ncomp) {
  for (int n = 0; n < N; ++n) {
    const vunet_jpeg_img& m = h[n];
    vunet_jpeg_info I;
    if (encode_info(m.height, m.width, m.ncomp, m.hsamp, m.vsamp, &I) != VUNET_OK) return false;
    if ((ncomp && m.ncomp != ncomp) || m.bw0 != I.bw0 || m.bh0 != I.bh0 || m.bw1 != I.bw1 || m.bh1 != I.bh1) return false;
  }
  return true;
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

// The four Huffman tables of a stream in DHT order -- DC0, AC0, DC1, AC1 -- as code counts per length 1 .. 16 and symbols.
// Annex K's, or the caller's: counts [4][16] and symbols [4][256] (a gray image reads the first two of each).
struct Tables {
  const uint8_t* counts[4];
  const uint8_t* symbols[4];
  int total[4];
};

inline Tables std_tables() {
  return Tables{{kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits}, {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals}, {12, 162, 12, 162}};
}

// caller's tables: every code fits its length (the counts are a prefix code's), at most 256 symbols, no symbol twice
inline bool caller_tables(const uint8_t* counts, const uint8_t* symbols, int ntab, Tables& t) {
  for (int k = 0; k < ntab; ++k) {
    const uint8_t* c = counts + 16 * k;
    const uint8_t* v = symbols + 256 * k;
    uint32_t code = 0;
    int total = 0;
    for (int len = 1; len <= 16; ++len) {
      code += c[len - 1];
      total += c[len - 1];
      if (code > (1u << len)) return false;
      code <<= 1;
    }
    if (total > 256) return false;
    bool seen[256] = {};
    for (int i = 0; i < total; ++i) {
      if (seen[v[i]]) return false;
      seen[v[i]] = true;
    }
    t.counts[k] = c;
    t.symbols[k] = v;
    t.total[k] = total;
  }
  return true;
}

// the tables as the device coder reads them: codes [ntab][256], len << 16 | code, 0 = no such symbol
inline void code_words(const Tables& t, int ntab, uint32_t* codes) {
  for (int k = 0; k < ntab; ++k) {
    Codes c;
    build_codes(t.counts[k], t.symbols[k], c);
    for (int i = 0; i < 256; ++i) codes[256 * k + i] = ((uint32_t)c.len[i] << 16) | c.code[i];
  }
}

inline bool encode_args_ok(const vunet_jpeg_info* info, const uint16_t* qtab) {
  if (!info || !qtab || !encode_info_ok(*info)) return false;
  for (int i = 0; i < 64 * info->ncomp; ++i)
    if (qtab[i] < 1 || qtab[i] > 255) return false;
  return info->ncomp != 3 || memcmp(qtab + 64, qtab + 128, 64 * sizeof(uint16_t)) == 0;
}

// SOI .. SOS: everything in front of the scan's bytes
inline void put_header(Sink& s, const vunet_jpeg_info& I, const uint16_t* qtab, const Tables& t) {
  const int ntab = I.ncomp == 3 ? 2 : 1;
  s.put16(0xFFD8);
  static const uint8_t app0[18] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  s.put_bytes(app0, 18);
  for (int k = 0; k < ntab; ++k) {
    s.put16(0xFFDB);
    s.put16(67);
    s.put(k);
    for (int i = 0; i < 64; ++i) s.put(qtab[64 * k + kZigzag[i]]);
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
  static const int ids[4] = {0x00, 0x10, 0x01, 0x11};
  for (int k = 0; k < 2 * ntab; ++k) put_dht(s, ids[k], t.counts[k], t.symbols[k], t.total[k]);
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
}

// counts / symbols NULL (both): Annex K's tables
inline int write_header(const vunet_jpeg_info* info, const uint16_t* qtab, const uint8_t* counts, const uint8_t* symbols, uint8_t* out,
                        int64_t cap, int64_t* len) {
  if (!out || !len || cap < 0 || !encode_args_ok(info, qtab) || !counts != !symbols) return VUNET_ERR_ARG;
  *len = 0;
  Tables t = std_tables();
  if (counts && !caller_tables(counts, symbols, info->ncomp == 3 ? 4 : 2, t)) return VUNET_ERR_ARG;
  Sink s{out, cap};
  put_header(s, *info, qtab, t);
  *len = s.n;
  return s.n > cap ? VUNET_JPEG_ERR_CAPACITY : VUNET_OK;
}

// The one walk over an image's blocks in scan order: MCUs left to right, top to bottom; per MCU the blocks component by component,
// row-major.  `on_dc(table, size, diff)` and `on_ac(table, symbol, size, value)` see exactly the symbols the coder emits -- the DC
// difference's bit length; one 0xF0 per 16 zeros of a run (size 0), (run << 4) | size per non-zero term, 0x00 where the block does
// not end at position 63 -- and return false to stop (a symbol their table lacks).  `table`: 0 for luma, 1 for chroma.
template <class Dc, class Ac>
inline int walk_blocks(const int16_t* coef, const vunet_jpeg_info& I, Dc&& on_dc, Ac&& on_ac) {
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
        const int t = c ? 1 : 0;
        for (int by = 0; by < nv[c]; ++by) {
          for (int bx = 0; bx < nh[c]; ++bx) {
            const int16_t* blk = base[c] + 64 * ((int64_t)(my * nv[c] + by) * bw[c] + (mx * nh[c] + bx));
            const int32_t diff = (int32_t)blk[0] - pred[c];
            pred[c] = blk[0];
            int nb = bit_length((uint32_t)(diff < 0 ? -diff : diff));
            if (nb > 11) return VUNET_JPEG_ERR_RANGE;
            if (!on_dc(t, nb, diff)) return VUNET_ERR_ARG;
            int run = 0;
            for (int k = 1; k < 64; ++k) {
              const int32_t v = blk[kZigzag[k]];
              if (v == 0) {
                ++run;
                continue;
              }
              for (; run > 15; run -= 16)
                if (!on_ac(t, 0xF0, 0, 0)) return VUNET_ERR_ARG;
              nb = bit_length((uint32_t)(v < 0 ? -v : v));
              if (nb > 10) return VUNET_JPEG_ERR_RANGE;
              if (!on_ac(t, (run << 4) | nb, nb, v)) return VUNET_ERR_ARG;
              run = 0;
            }
            if (run && !on_ac(t, 0x00, 0, 0)) return VUNET_ERR_ARG;
          }
        }
      }
    }
  }
  return VUNET_OK;
}

// hist [4][256] in DHT order (DC0, AC0, DC1, AC1; a gray image leaves the last two zero): how often the coder emits each symbol
inline int symbol_histogram(const int16_t* coef, const vunet_jpeg_info* info, uint32_t* hist) {
  if (!coef || !info || !hist || !encode_info_ok(*info)) return VUNET_ERR_ARG;
  memset(hist, 0, 4 * 256 * sizeof(uint32_t));
  return walk_blocks(
      coef, *info,
      [&](int t, int nb, int32_t) {
        ++hist[512 * t + nb];
        return true;
      },
      [&](int t, int sym, int, int32_t) {
        ++hist[512 * t + 256 + sym];
        return true;
      });
}

// libjpeg's jpeg_gen_optimal_table (jchuff.c), restated: freq [256] -> the code counts per length 1 .. 16 and the symbols, ordered
// by length and within a length by value; *nsym of them.  Symbol 256 is a reserved code point of frequency 1, so that no code is all
// ones; it always ends up among the longest codes and is taken away last.  Code lengths above 16 are shortened pairwise
// (section K.2's procedure).  A code that would need more than 32 bits before that is VUNET_ERR_ARG, as libjpeg refuses it.
inline int optimal_table(const uint32_t* freq_in, uint8_t* counts, uint8_t* symbols, int32_t* nsym) {
  if (!freq_in || !counts || !symbols || !nsym) return VUNET_ERR_ARG;
  constexpr int kMaxLen = 32;
  int64_t freq[257];
  int codesize[257], others[257];
  int long_bits[kMaxLen + 1] = {};
  for (int i = 0; i < 256; ++i) freq[i] = freq_in[i];
  freq[256] = 1;
  for (int i = 0; i < 257; ++i) {
    codesize[i] = 0;
    others[i] = -1;
  }
  for (;;) {
    // the two smallest non-zero frequencies, ties to the larger index
    int c1 = -1, c2 = -1;
    int64_t v = INT64_MAX;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] <= v) {
        v = freq[i];
        c1 = i;
      }
    v = INT64_MAX;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] <= v && i != c1) {
        v = freq[i];
        c2 = i;
      }
    if (c2 < 0) break;
    freq[c1] += freq[c2];
    freq[c2] = 0;
    for (++codesize[c1]; others[c1] >= 0;) {
      c1 = others[c1];
      ++codesize[c1];
    }
    others[c1] = c2;
    for (++codesize[c2]; others[c2] >= 0;) {
      c2 = others[c2];
      ++codesize[c2];
    }
  }
  for (int i = 0; i <= 256; ++i)
    if (codesize[i]) {
      if (codesize[i] > kMaxLen) return VUNET_ERR_ARG;
      ++long_bits[codesize[i]];
    }
  for (int i = kMaxLen; i > 16; --i)
    while (long_bits[i] > 0) {
      int j = i - 2;
      while (long_bits[j] == 0) --j;
      long_bits[i] -= 2;
      ++long_bits[i - 1];
      long_bits[j + 1] += 2;
      --long_bits[j];
    }
  int last = 16;
  while (last > 0 && long_bits[last] == 0) --last;
  if (last > 0) --long_bits[last];   // (no symbol at all: an empty table)
  for (int i = 1; i <= 16; ++i) counts[i - 1] = (uint8_t)long_bits[i];
  int p = 0;
  for (int len = 1; len <= kMaxLen; ++len)
    for (int j = 0; j < 256; ++j)
      if (codesize[j] == len) symbols[p++] = (uint8_t)j;
  *nsym = p;
  return VUNET_OK;
}

// A batch's tables from its histograms, as the device route needs them between two launches: hist [N][4][256] -> counts [N][4][16],
// symbols [N][4][256] and codes [N][4][256] (code_words' form); the first `ntab` (2 or 4) tables of an image are built, the others
// are empty.  -> the first code that is not VUNET_OK, *failed the image it belongs to
inline int optimal_tables(const uint32_t* hist, int32_t N, int32_t ntab, uint8_t* counts, uint8_t* symbols, uint32_t* codes,
                          int32_t* failed) {
  if (!hist || !counts || !symbols || !codes || !failed || N < 1 || (ntab != 2 && ntab != 4)) return VUNET_ERR_ARG;
  memset(counts, 0, (size_t)N * 64);
  memset(symbols, 0, (size_t)N * 1024);
  for (int n = 0; n < N; ++n) {
    uint8_t* c = counts + (size_t)n * 64;
    uint8_t* s = symbols + (size_t)n * 1024;
    *failed = n;
    for (int t = 0; t < ntab; ++t) {
      int32_t nsym = 0;
      const int rc = optimal_table(hist + (size_t)n * 1024 + 256 * t, c + 16 * t, s + 256 * t, &nsym);
      if (rc != VUNET_OK) return rc;
    }
    Tables T;
    if (!caller_tables(c, s, 4, T)) return VUNET_ERR_ARG;
    code_words(T, 4, codes + (size_t)n * 1024);
  }
  *failed = -1;
  return VUNET_OK;
}

// counts / symbols NULL (both): Annex K's tables, the stream vunet_jpeg_entropy_encode writes.  A symbol the caller's tables lack
// is VUNET_ERR_ARG (*len is then 0).
inline int entropy_encode_tables(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, const uint8_t* counts,
                                 const uint8_t* symbols, uint8_t* out, int64_t cap, int64_t* len) {
  if (!coef || !out || !len || cap < 0 || !encode_args_ok(info, qtab) || !counts != !symbols) return VUNET_ERR_ARG;
  *len = 0;
  const vunet_jpeg_info& I = *info;
  Tables t = std_tables();
  if (counts && !caller_tables(counts, symbols, I.ncomp == 3 ? 4 : 2, t)) return VUNET_ERR_ARG;
  Sink s{out, cap};
  put_header(s, I, qtab, t);
  Codes dc[2], ac[2];
  for (int k = 0; k < (I.ncomp == 3 ? 2 : 1); ++k) {
    build_codes(t.counts[2 * k], t.symbols[2 * k], dc[k]);
    build_codes(t.counts[2 * k + 1], t.symbols[2 * k + 1], ac[k]);
  }
  const int rc = walk_blocks(
      coef, I,
      [&](int k, int nb, int32_t diff) {
        const Codes& h = dc[k];
        if (!h.len[nb]) return false;
        s.put_bits(h.code[nb], h.len[nb]);
        if (nb) s.put_bits((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << nb) - 1), nb);
        return true;
      },
      [&](int k, int sym, int nb, int32_t v) {
        const Codes& h = ac[k];
        if (!h.len[sym]) return false;
        s.put_bits(((uint32_t)h.code[sym] << nb) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << nb) - 1)), h.len[sym] + nb);
        return true;
      });
  if (rc != VUNET_OK) return rc;
  s.flush_bits();
  s.put16(0xFFD9);
  *len = s.n;
  return s.n > cap ? VUNET_JPEG_ERR_CAPACITY : VUNET_OK;
}

// The device coder's spans, one (offset, bits) pair per image: where the image's unstuffed scan bytes start in `raw` and how many
// bits they are.  The images lie one after the other, each from a multiple of kStuffChunk: the pairs must say exactly that, no
// image may have more bits than its blocks can code to (or than 32 bits count), and the buffers must hold what follows from them:
// `raw` every chunk, `out` two bytes per unstuffed byte (every byte stuffed), `chunks` one word per chunk.  -> *nchunks
inline bool spans_ok(const int64_t* spans, const vunet_jpeg_img* h, int N, int64_t raw_bytes, int64_t out_cap, int64_t chunk_count,
                     int64_t* nchunks) {
  int64_t at = 0, out = 0;
  for (int n = 0; n < N; ++n) {
    const int64_t nb = (int64_t)h[n].bw0 * h[n].bh0 + 2 * (int64_t)h[n].bw1 * h[n].bh1, bits = spans[2 * n + 1];
    if (spans[2 * n] != at || bits < 1 || bits > nb * kBlockBits || bits > 0xFFFFFFFFll) return false;
    const int64_t bytes = (bits + 7) / 8;
    at += (bytes + kStuffChunk - 1) / kStuffChunk * kStuffChunk;
    out += 2 * bytes;
  }
  if (at > raw_bytes || out > out_cap || out > 0xFFFFFFFFll || at / kStuffChunk > chunk_count) return false;
  *nchunks = at / kStuffChunk;
  return true;
}

inline int entropy_encode(const int16_t* coef, const vunet_jpeg_info* info, const uint16_t* qtab, uint8_t* out, int64_t cap,
                          int64_t* len) {
  return entropy_encode_tables(coef, info, qtab, nullptr, nullptr, out, cap, len);
}

}  // namespace vunet_jpeg

