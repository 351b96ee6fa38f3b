// The host half of the baseline JPEG decoder: the marker parse and the Huffman walk.  Plain C++17, no HIP, header-only; included by
// jpeg.hip (the C ABI of include/vunet_jpeg.h) and by tools/jpeg_host_check.cpp.  The bytes are untrusted: every read is checked
// against `len`, every table against its size, every coefficient index against its block, and nothing is written outside the
// info's ncoef coefficients and ncomp * 64 table entries.  Errors are the VUNET_JPEG_ERR_* codes; nothing throws.
//
// The bit reader keeps up to 64 bits and stops filling at a marker or at the end of the data; from there it feeds zero bits and
// counts them, and a block that consumed one of those is an error (the stream is truncated or a marker cut the scan short).  So no
// Huffman look-up ever needs a bounds check of its own.  Codes of up to 9 bits are resolved by one table look-up, longer ones by
// the canonical maxcode walk (as libjpeg does).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/vunet_hip.h"
#include "../../include/vunet_jpeg.h"
#include "../../include/vunet_jpeg_huffdec.h"
#include "jpeg_sync.h"

namespace vunet_jpeg {

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int kLook = 9;

struct Huff {
  bool defined = false;
  uint8_t symbols[256];
  int32_t maxcode[18];    // largest code of each length, -1 if none; [17] ends every walk
  int32_t valoff[17];     // symbols index of the first code of a length, minus that code
  uint16_t look[1 << kLook];   // (length << 8) | symbol for codes of <= kLook bits, 0 otherwise
};

struct Header {
  vunet_jpeg_info info;
  uint16_t qt[4][64];     // natural order
  bool qt_defined[4] = {false, false, false, false};
  Huff huff[2][4];        // [dc / ac][table]
  int tq[3], td[3], ta[3];
  int64_t scan;           // offset of the entropy-coded data
};

// counts[16] and the symbols of one DHT table -> the decoding tables; false where the code lengths overflow the code space
inline bool build_huff(const uint8_t* counts, const uint8_t* symbols, int total, Huff& h) {
  memset(h.look, 0, sizeof(h.look));
  memcpy(h.symbols, symbols, (size_t)total);
  int32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    const int n = counts[len - 1];
    if (code + n > (1 << len)) return false;
    h.valoff[len] = k - code;
    if (n) {
      if (len <= kLook)
        for (int i = 0; i < n; ++i) {
          const int first = (code + i) << (kLook - len);
          for (int j = 0; j < (1 << (kLook - len)); ++j) h.look[first + j] = (uint16_t)((len << 8) | symbols[k + i]);
        }
      k += n;
      code += n;
      h.maxcode[len] = code - 1;
    } else {
      h.maxcode[len] = -1;
    }
    code <<= 1;
  }
  h.maxcode[17] = 0x7FFFFFFF;
  h.defined = true;
  return true;
}

inline int parse(const uint8_t* d, int64_t len, Header& H) {
  if (!d || len < 0) return VUNET_ERR_ARG;
  if (len < 2) return VUNET_JPEG_ERR_TRUNCATED;
  if (d[0] != 0xFF || d[1] != 0xD8) return VUNET_JPEG_ERR_MARKER;
  int64_t p = 2;
  bool have_frame = false, jfif = false;
  int adobe = -1, ncomp = 0, height = 0, width = 0, restart = 0;
  int cid[3] = {0, 0, 0}, ch[3] = {0, 0, 0}, cv[3] = {0, 0, 0};
  for (;;) {
    if (p >= len) return VUNET_JPEG_ERR_TRUNCATED;
    if (d[p] != 0xFF) return VUNET_JPEG_ERR_MARKER;
    while (p < len && d[p] == 0xFF) ++p;
    if (p >= len) return VUNET_JPEG_ERR_TRUNCATED;
    const int m = d[p++];
    if (m == 0xD9 || m == 0xD8 || m == 0 || (m >= 0xD0 && m <= 0xD7)) return VUNET_JPEG_ERR_MARKER;
    if (m == 0x01) continue;
    if (p + 2 > len) return VUNET_JPEG_ERR_TRUNCATED;
    const int n = (d[p] << 8) | d[p + 1];
    if (n < 2) return VUNET_JPEG_ERR_MARKER;
    if (p + n > len) return VUNET_JPEG_ERR_TRUNCATED;
    const uint8_t* seg = d + p + 2;
    const int sl = n - 2;
    p += n;
    if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, t = seg[q] & 15;
        if (pq != 0) return VUNET_JPEG_ERR_PRECISION;
        if (t > 3 || q + 65 > sl) return VUNET_JPEG_ERR_MARKER;
        for (int i = 0; i < 64; ++i) H.qt[t][kZigzag[i]] = seg[q + 1 + i];
        H.qt_defined[t] = true;
        q += 65;
      }
    } else if (m == 0xC0) {
      if (sl < 6) return VUNET_JPEG_ERR_MARKER;
      if (seg[0] != 8) return VUNET_JPEG_ERR_PRECISION;
      height = (seg[1] << 8) | seg[2];
      width = (seg[3] << 8) | seg[4];
      ncomp = seg[5];
      if (ncomp != 1 && ncomp != 3) return VUNET_JPEG_ERR_COMPONENTS;
      if (sl != 6 + 3 * ncomp || height < 1 || width < 1 || have_frame) return VUNET_JPEG_ERR_MARKER;
      for (int i = 0; i < ncomp; ++i) {
        cid[i] = seg[6 + 3 * i];
        ch[i] = seg[7 + 3 * i] >> 4;
        cv[i] = seg[7 + 3 * i] & 15;
        H.tq[i] = seg[8 + 3 * i];
      }
      have_frame = true;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
      return VUNET_JPEG_ERR_SOF;
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        if (tc > 1 || th > 3 || q + 17 > sl) return VUNET_JPEG_ERR_MARKER;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += seg[q + 1 + i];
        if (total > 256 || q + 17 + total > sl) return VUNET_JPEG_ERR_MARKER;
        if (!build_huff(seg + q + 1, seg + q + 17, total, H.huff[tc][th])) return VUNET_JPEG_ERR_MARKER;
        q += 17 + total;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return VUNET_JPEG_ERR_MARKER;
      restart = (seg[0] << 8) | seg[1];
    } else if (m == 0xE0 && sl >= 5 && memcmp(seg, "JFIF\0", 5) == 0) {
      jfif = true;
    } else if (m == 0xEE && sl >= 12 && memcmp(seg, "Adobe", 5) == 0) {
      adobe = seg[11];
    } else if (m == 0xDA) {
      if (!have_frame || sl < 1) return VUNET_JPEG_ERR_MARKER;
      const int ns = seg[0];
      if (ns != ncomp) return (ns >= 1 && ns < ncomp) ? VUNET_JPEG_ERR_SCANS : VUNET_JPEG_ERR_MARKER;
      if (sl != 4 + 2 * ns) return VUNET_JPEG_ERR_MARKER;
      for (int i = 0; i < ns; ++i) {
        if (seg[1 + 2 * i] != cid[i]) return VUNET_JPEG_ERR_MARKER;
        H.td[i] = seg[2 + 2 * i] >> 4;
        H.ta[i] = seg[2 + 2 * i] & 15;
      }
      if (seg[1 + 2 * ns] != 0 || seg[2 + 2 * ns] != 63 || seg[3 + 2 * ns] != 0) return VUNET_JPEG_ERR_MARKER;
      break;
    }
    // every other segment (APPn, COM, ...) is skipped
  }
  int hs = 1, vs = 1;
  if (ncomp == 3) {
    if (adobe >= 0 && adobe != 1) return VUNET_JPEG_ERR_COMPONENTS;
    if (adobe < 0 && !jfif && cid[0] == 82 && cid[1] == 71 && cid[2] == 66) return VUNET_JPEG_ERR_COMPONENTS;
    hs = ch[0];
    vs = cv[0];
    if (!((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2)) || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 ||
        cv[2] != 1)
      return VUNET_JPEG_ERR_SAMPLING;
  } else if (ch[0] < 1 || cv[0] < 1) {
    return VUNET_JPEG_ERR_MARKER;
  }
  for (int i = 0; i < ncomp; ++i) {
    if (H.tq[i] > 3 || !H.qt_defined[H.tq[i]] || H.td[i] > 3 || H.ta[i] > 3 || !H.huff[0][H.td[i]].defined ||
        !H.huff[1][H.ta[i]].defined)
      return VUNET_JPEG_ERR_MARKER;
  }
  vunet_jpeg_info& I = H.info;
  I.height = height;
  I.width = width;
  I.ncomp = ncomp;
  I.hsamp = hs;
  I.vsamp = vs;
  I.mcu_cols = (width + 8 * hs - 1) / (8 * hs);
  I.mcu_rows = (height + 8 * vs - 1) / (8 * vs);
  I.restart = restart;
  I.bw0 = I.mcu_cols * hs;
  I.bh0 = I.mcu_rows * vs;
  I.bw1 = ncomp == 3 ? I.mcu_cols : 0;
  I.bh1 = ncomp == 3 ? I.mcu_rows : 0;
  I.nblocks = I.bw0 * I.bh0 + 2 * I.bw1 * I.bh1;   // (at most 8192 * 8192 * 3 / 2: fits)
  if (I.nblocks > (0x7FFFFFFF >> 6)) return VUNET_JPEG_ERR_MARKER;
  I.ncoef = I.nblocks * 64;
  H.scan = p;
  return VUNET_OK;
}

struct Bits {
  const uint8_t* d;
  int64_t p, len;
  uint64_t acc = 0;
  int n = 0;        // bits in acc
  int zeros = 0;    // how many of them are padding fed after a marker or the end of the data
  bool stopped = false;

  inline void fill() {
    while (n <= 56) {
      int b = 0;
      if (!stopped) {
        if (p >= len) {
          stopped = true;
        } else if (d[p] == 0xFF) {
          if (p + 1 < len && d[p + 1] == 0) {
            b = 0xFF;
            p += 2;
          } else {
            stopped = true;   // a marker, or the data ends inside one: p stays on its 0xFF
          }
        } else {
          b = d[p++];
        }
      }
      if (stopped) zeros += 8;
      acc = (acc << 8) | (uint64_t)b;
      n += 8;
    }
  }
  inline int peek(int k) { return (int)((acc >> (n - k)) & ((1u << k) - 1)); }   // n >= k is the caller's
  inline void skip(int k) { n -= k; }
  inline int get(int k) {
    if (k == 0) return 0;
    const int v = peek(k);
    n -= k;
    return v;
  }
  inline bool overrun() const { return n < zeros; }
};

// one Huffman symbol, or -1 (no such code).  Needs n >= 16 (fill() guarantees 57)
inline int symbol(Bits& br, const Huff& h) {
  const int e = h.look[br.peek(kLook)];
  if (e) {
    br.skip(e >> 8);
    return e & 0xFF;
  }
  int len = kLook + 1;
  int32_t code = br.peek(len);
  while (len <= 16 && code > h.maxcode[len]) {
    ++len;
    code = br.peek(len);
  }
  if (len > 16) return -1;
  br.skip(len);
  const int idx = h.valoff[len] + code;
  return (idx >= 0 && idx < 256) ? h.symbols[idx] : -1;
}

inline int extend(int v, int s) { return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1; }

// what ended the data early: the end of the stream, or a marker inside the scan
inline int scan_error(const Bits& br) { return br.p + 1 >= br.len ? VUNET_JPEG_ERR_TRUNCATED : VUNET_JPEG_ERR_MARKER; }

inline bool same_info(const vunet_jpeg_info& a, const vunet_jpeg_info& b) {
  return a.height == b.height && a.width == b.width && a.ncomp == b.ncomp && a.hsamp == b.hsamp && a.vsamp == b.vsamp &&
         a.mcu_cols == b.mcu_cols && a.mcu_rows == b.mcu_rows && a.restart == b.restart && a.bw0 == b.bw0 && a.bh0 == b.bh0 &&
         a.bw1 == b.bw1 && a.bh1 == b.bh1 && a.nblocks == b.nblocks && a.ncoef == b.ncoef;
}

inline int parse_info(const uint8_t* d, int64_t len, vunet_jpeg_info* info) {
  if (!d || !info || len < 0) return VUNET_ERR_ARG;
  Header* H = new Header();
  const int rc = parse(d, len, *H);
  if (rc == VUNET_OK) *info = H->info;
  delete H;
  return rc;
}

inline int entropy_decode(const uint8_t* d, int64_t len, const vunet_jpeg_info* info, int16_t* coef, uint16_t* qtab) {
  if (!d || !info || !coef || !qtab || len < 0) return VUNET_ERR_ARG;
  Header* Hp = new Header();
  struct Free {
    Header* h;
    ~Free() { delete h; }
  } guard{Hp};
  Header& H = *Hp;
  int rc = parse(d, len, H);
  if (rc != VUNET_OK) return rc;
  const vunet_jpeg_info& I = H.info;
  if (!same_info(I, *info)) return VUNET_ERR_ARG;
  for (int c = 0; c < I.ncomp; ++c) memcpy(qtab + 64 * c, H.qt[H.tq[c]], 64 * sizeof(uint16_t));
  memset(coef, 0, (size_t)I.ncoef * sizeof(int16_t));
  int16_t* base[3];
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
  Bits br{d, H.scan, len};
  uint32_t pred[3] = {0, 0, 0};   // (modular: a corrupt stream may run the prediction anywhere)
  int nrst = 0, left = I.restart;
  for (int my = 0; my < I.mcu_rows; ++my) {
    for (int mx = 0; mx < I.mcu_cols; ++mx) {
      if (I.restart && left == 0) {
        // the rest of the byte is padding; the marker must be next (fill() stopped on it: no later byte is in acc)
        br.fill();
        if (!br.stopped || br.n - br.zeros >= 8) return VUNET_JPEG_ERR_RESTART;
        int64_t p = br.p;
        while (p < len && d[p] == 0xFF) ++p;
        if (p >= len) return VUNET_JPEG_ERR_TRUNCATED;
        if (p == br.p || d[p] != 0xD0 + (nrst & 7)) return VUNET_JPEG_ERR_RESTART;
        br = Bits{d, p + 1, len};
        ++nrst;
        left = I.restart;
        pred[0] = pred[1] = pred[2] = 0;
      }
      --left;
      for (int c = 0; c < I.ncomp; ++c) {
        const Huff& hd = H.huff[0][H.td[c]];
        const Huff& ha = H.huff[1][H.ta[c]];
        for (int by = 0; by < nv[c]; ++by) {
          for (int bx = 0; bx < nh[c]; ++bx) {
            int16_t* blk = base[c] + 64 * ((int64_t)(my * nv[c] + by) * bw[c] + (mx * nh[c] + bx));
            br.fill();
            int s = symbol(br, hd);
            if (s < 0 || s > 15) return br.overrun() ? scan_error(br) : VUNET_JPEG_ERR_HUFFMAN;
            pred[c] += (uint32_t)extend(br.get(s), s);
            blk[0] = (int16_t)(uint16_t)pred[c];
            int k = 1;
            while (k < 64) {
              br.fill();
              const int rs = symbol(br, ha);
              if (rs < 0) return br.overrun() ? scan_error(br) : VUNET_JPEG_ERR_HUFFMAN;
              const int r = rs >> 4;
              s = rs & 15;
              if (s == 0) {
                if (r != 15) break;
                k += 16;
                continue;
              }
              k += r;
              if (k > 63) return br.overrun() ? scan_error(br) : VUNET_JPEG_ERR_HUFFMAN;
              blk[kZigzag[k]] = (int16_t)extend(br.get(s), s);
              ++k;
            }
            if (br.overrun()) return scan_error(br);
          }
        }
      }
    }
  }
  // what follows the scan: EOI, or this stream is not the one-scan kind / is cut short
  int64_t p = br.p;
  if (!br.stopped) {
    br.fill();
    if (!br.stopped) {
      // (bytes of entropy-coded data are left over: walk to the next marker as libjpeg does)
      p = br.p;
      while (p < len && !(d[p] == 0xFF && p + 1 < len && d[p + 1] != 0 && d[p + 1] != 0xFF)) ++p;
    } else {
      p = br.p;
    }
  }
  while (p < len && d[p] == 0xFF) ++p;
  if (p >= len) return VUNET_JPEG_ERR_TRUNCATED;
  if (d[p] == 0xD9) return VUNET_OK;
  if (d[p] == 0xDA || d[p] == 0xC4 || d[p] == 0xDB) return VUNET_JPEG_ERR_SCANS;
  return VUNET_JPEG_ERR_MARKER;
}

// ---- the host side of the device entropy decoder (jpeg_huff_dec.hip): no bit walk, a byte-level marker scan

// the stream's decoding tables as one device row; false where more than two DC or two AC tables are in use.  The row is a valid
// one either way (the MCU's shape is the image's, every table index is in range): such a stream brings no subsequences, but its
// row travels with the batch's and is checked with them
inline bool flatten_tables(const Header& H, vunet_jpeg_sync::Tables& T) {
  memset(&T, 0, sizeof(T));
  const vunet_jpeg_info& I = H.info;
  T.hv = I.ncomp == 3 ? I.hsamp * I.vsamp : 1;
  T.per_mcu = I.ncomp == 3 ? T.hv + 2 : 1;
  T.restart = I.restart;
  int ids[2][2] = {{-1, -1}, {-1, -1}};
  for (int c = 0; c < I.ncomp; ++c)
    for (int kind = 0; kind < 2; ++kind) {
      const int id = kind ? H.ta[c] : H.td[c];
      int slot = ids[kind][0] == id ? 0 : (ids[kind][1] == id ? 1 : -1);
      if (slot < 0) {
        slot = ids[kind][0] < 0 ? 0 : (ids[kind][1] < 0 ? 1 : -1);
        if (slot < 0) return false;
        ids[kind][slot] = id;
        const Huff& h = H.huff[kind][id];
        vunet_jpeg_sync::Table& t = T.t[2 * kind + slot];
        memcpy(t.look, h.look, sizeof(t.look));
        memcpy(t.maxcode, h.maxcode, sizeof(t.maxcode));
        memcpy(t.symbols, h.symbols, sizeof(t.symbols));
        for (int len = 1; len <= 16; ++len) t.valoff[len] = h.valoff[len];
      }
      (kind ? T.ac : T.dc)[c] = 2 * kind + slot;
    }
  return true;
}

inline int64_t expected_segments(const vunet_jpeg_info& I) {
  const int64_t mcus = (int64_t)I.mcu_cols * I.mcu_rows;
  return I.restart > 0 ? (mcus + I.restart - 1) / I.restart : 1;
}

inline int scan_segments(const uint8_t* d, int64_t len, const vunet_jpeg_info* info, int64_t* segs, int64_t seg_cap, int64_t* nseg,
                         uint16_t* qtab, uint8_t* tab) {
  if (!d || !info || !segs || !nseg || !qtab || !tab || len < 0) return VUNET_ERR_ARG;
  Header* Hp = new Header();
  struct Free {
    Header* h;
    ~Free() { delete h; }
  } guard{Hp};
  Header& H = *Hp;
  const int rc = parse(d, len, H);
  if (rc != VUNET_OK) return rc;
  const vunet_jpeg_info& I = H.info;
  if (!same_info(I, *info)) return VUNET_ERR_ARG;
  const int64_t expected = expected_segments(I);
  if (seg_cap < expected) return VUNET_ERR_ARG;
  *nseg = 0;
  for (int c = 0; c < I.ncomp; ++c) memcpy(qtab + 64 * c, H.qt[H.tq[c]], 64 * sizeof(uint16_t));
  vunet_jpeg_sync::Tables* T = new vunet_jpeg_sync::Tables();
  const bool flat = flatten_tables(H, *T);
  memcpy(tab, T, sizeof(*T));
  delete T;
  if (!flat) return VUNET_JPEG_HUFFDEC_IRREGULAR;
  int64_t p = H.scan, begin = H.scan, count = 0;
  for (;;) {
    const uint8_t* q = p < len ? (const uint8_t*)memchr(d + p, 0xFF, (size_t)(len - p)) : nullptr;
    if (!q) return VUNET_JPEG_HUFFDEC_IRREGULAR;              // no EOI
    p = q - d;
    if (p + 1 >= len) return VUNET_JPEG_HUFFDEC_IRREGULAR;    // an FF at the end of the data
    const int m = d[p + 1];
    if (m == 0) {
      p += 2;
      continue;
    }
    const bool rst = m >= 0xD0 && m <= 0xD7;
    if (!rst && m != 0xD9) return VUNET_JPEG_HUFFDEC_IRREGULAR;   // fill bytes, any other marker
    if (p == begin || count >= expected) return VUNET_JPEG_HUFFDEC_IRREGULAR;
    if (rst && (I.restart == 0 || m != 0xD0 + (int)(count & 7))) return VUNET_JPEG_HUFFDEC_IRREGULAR;
    segs[3 * count] = begin;
    segs[3 * count + 1] = p;
    segs[3 * count + 2] = count * (int64_t)I.restart;
    ++count;
    if (!rst) break;
    begin = p = p + 2;
  }
  if (count != expected) return VUNET_JPEG_HUFFDEC_IRREGULAR;
  *nseg = count;
  return VUNET_OK;
}

inline int subseq_rows(const int64_t* segs, int64_t nseg, const vunet_jpeg_info* info, int32_t img, int64_t byte_off, int64_t row0,
                       vunet_jpeg_subseq* rows, int64_t row_cap, int64_t* nrows, int64_t subseq_bytes = VUNET_JPEG_SUBSEQ_BYTES) {
  if (!segs || !info || !rows || !nrows || nseg < 1 || img < 0 || row0 < 0 || row0 % VUNET_JPEG_HUFFDEC_GROUP || subseq_bytes < 8)
    return VUNET_ERR_ARG;
  const vunet_jpeg_info& I = *info;
  const int64_t per_mcu = I.ncomp == 3 ? I.hsamp * I.vsamp + 2 : 1, mcus = (int64_t)I.mcu_cols * I.mcu_rows;
  int64_t at = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t b = segs[3 * s] + byte_off, e = segs[3 * s + 1] + byte_off, mcu0 = segs[3 * s + 2];
    if (b < 0 || e <= b || e > VUNET_JPEG_HUFFDEC_MAX_BYTES || mcu0 < 0 || mcu0 >= mcus) return VUNET_ERR_ARG;
    const int64_t in_seg = I.restart > 0 && mcus - mcu0 > I.restart ? I.restart : mcus - mcu0;
    const int64_t n = (e - b + subseq_bytes - 1) / subseq_bytes;
    if (at + n > row_cap || row0 + at + n > 0x7FFFFFFF) return VUNET_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) {
      vunet_jpeg_subseq& r = rows[at + i];
      r.img = img;
      r.seg_begin = (int32_t)b;
      r.seg_end = (int32_t)e;
      r.begin = (int32_t)(b + i * subseq_bytes);
      r.end = (int32_t)(i + 1 == n ? e : b + (i + 1) * subseq_bytes);
      r.first_block = (int32_t)(mcu0 * per_mcu);
      r.seg_blocks = (int32_t)(in_seg * per_mcu);
      r.seg_row = (int32_t)(row0 + at);
      r.flags = (i == 0 ? VUNET_JPEG_SUBSEQ_FIRST : 0) | (i + 1 == n ? VUNET_JPEG_SUBSEQ_LAST : 0) |
                (s + 1 == nseg ? VUNET_JPEG_SUBSEQ_TAIL : 0);
      r.reserved = 0;
    }
    at += n;
  }
  const int64_t padded = (at + VUNET_JPEG_HUFFDEC_GROUP - 1) / VUNET_JPEG_HUFFDEC_GROUP * VUNET_JPEG_HUFFDEC_GROUP;
  if (padded > row_cap) return VUNET_ERR_ARG;
  for (; at < padded; ++at) {
    memset(&rows[at], 0, sizeof(rows[at]));
    rows[at].img = img;
    rows[at].flags = VUNET_JPEG_SUBSEQ_PAD;
  }
  *nrows = padded;
  return VUNET_OK;
}

// every row of the host copy against the buffers and against its neighbours: nothing is launched on rows that could make a
// kernel read outside `bytes`, take another image's tables or index outside `state`
inline bool subseq_rows_ok(const vunet_jpeg_subseq* h, int64_t nsub, int64_t bytes_count, const vunet_jpeg_img* imgs, int N,
                           int64_t subseq_bytes = VUNET_JPEG_SUBSEQ_BYTES) {
  if (nsub < VUNET_JPEG_HUFFDEC_GROUP || nsub % VUNET_JPEG_HUFFDEC_GROUP || nsub > 0x7FFFFFFF / 16) return false;
  if (bytes_count < 0 || bytes_count > VUNET_JPEG_HUFFDEC_MAX_BYTES) return false;
  for (int64_t i = 0; i < nsub; ++i) {
    const vunet_jpeg_subseq& r = h[i];
    const vunet_jpeg_subseq& lead = h[i - i % VUNET_JPEG_HUFFDEC_GROUP];
    if (r.img < 0 || r.img >= N || r.img != lead.img) return false;
    if (r.flags & VUNET_JPEG_SUBSEQ_PAD) {
      if (i % VUNET_JPEG_HUFFDEC_GROUP == 0) return false;   // (a workgroup's first row names its image: never padding)
      continue;
    }
    if (r.flags & ~7) return false;
    const vunet_jpeg_img& m = imgs[r.img];
    const int64_t nb = (int64_t)m.bw0 * m.bh0 + 2 * (int64_t)m.bw1 * m.bh1;
    if (r.seg_begin < 0 || r.begin < r.seg_begin || r.end <= r.begin || r.seg_end < r.end || r.seg_end > bytes_count ||
        r.end - r.begin > subseq_bytes)
      return false;
    if (r.first_block < 0 || r.seg_blocks < 1 || (int64_t)r.first_block + r.seg_blocks > nb) return false;
    const bool first = r.flags & VUNET_JPEG_SUBSEQ_FIRST, last = r.flags & VUNET_JPEG_SUBSEQ_LAST;
    if (first != (r.begin == r.seg_begin) || last != (r.end == r.seg_end)) return false;
    if (first) {
      if (r.seg_row != i) return false;
    } else {
      if (i == 0) return false;
      const vunet_jpeg_subseq& p = h[i - 1];
      if ((p.flags & (VUNET_JPEG_SUBSEQ_PAD | VUNET_JPEG_SUBSEQ_LAST)) || p.img != r.img || p.seg_begin != r.seg_begin ||
          p.seg_end != r.seg_end || p.end != r.begin || p.seg_row != r.seg_row || p.first_block != r.first_block ||
          p.seg_blocks != r.seg_blocks || (p.flags & VUNET_JPEG_SUBSEQ_TAIL) != (r.flags & VUNET_JPEG_SUBSEQ_TAIL))
        return false;
    }
    if (!last) {
      if (i + 1 >= nsub || (h[i + 1].flags & (VUNET_JPEG_SUBSEQ_PAD | VUNET_JPEG_SUBSEQ_FIRST))) return false;
    }
  }
  return true;
}

// the host copy of the table rows against the images they belong to: every index a kernel takes from a row is in range
inline bool table_rows_ok(const uint8_t* tabs, const vunet_jpeg_img* imgs, int N) {
  for (int n = 0; n < N; ++n) {
    vunet_jpeg_sync::Tables* T = new vunet_jpeg_sync::Tables();
    memcpy(T, tabs + (size_t)n * sizeof(*T), sizeof(*T));
    const vunet_jpeg_img& m = imgs[n];
    const int hv = m.ncomp == 3 ? m.hsamp * m.vsamp : 1;
    bool ok = T->hv == hv && T->per_mcu == (m.ncomp == 3 ? hv + 2 : 1) && T->restart >= 0;
    for (int c = 0; c < 3; ++c) ok = ok && T->dc[c] >= 0 && T->dc[c] <= 3 && T->ac[c] >= 0 && T->ac[c] <= 3;
    delete T;
    if (!ok) return false;
  }
  return true;
}

}  // namespace vunet_jpeg
