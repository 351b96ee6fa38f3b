// The Huffman walk of the device entropy decoder (jpeg_huff_dec.hip), as one header that host and device share: plain C++17, no HIP
// call, no allocation, no recursion.  Under hipcc everything is __host__ __device__, under a host compiler it is host code, and
// tools/jpeg_sync_check.cpp runs exactly this walk on the CPU under the sanitizers.
//
// A scan without restart markers is one bit string, and a restart interval is one too.  Such a segment is cut into subsequences of
// a fixed number of bytes; one thread walks one subsequence.  The walk takes a parser state -- (bit position, block index within the
// MCU, zigzag index k; k = 0: the DC symbol is next) -- and returns the state at the first symbol boundary at or behind the
// subsequence's last bit, with the number of blocks BEGUN on the way (DC symbols decoded).  Huffman codes self-synchronise: a walk
// from a guessed state soon parses as the true one does, so iterating "my entry state is my predecessor's exit state" from a known
// first state reaches the true states.
//
// Positions are bit offsets into the STUFFED bytes, and never rest on a stuffed byte: the 00 behind an FF belongs to the FF.
// The bytes are untrusted and a guessed state parses garbage: every loop is bounded by the bits of the subsequence (each symbol
// takes at least one), every table index, block ordinal and coefficient index is checked before use, and no byte outside the
// segment [seg_begin, seg_end) is read.  Past seg_end the reader feeds zero bits and counts them (as jpeg_entropy.h's Bits does);
// a symbol that used one is not decoded -- the walk STOPs in front of it.
//
// A walk from a guessed state may meet a code that is in no table, a DC category above 15 or an index past 63.  That is normal and
// gives the canonical LOST state (the subsequence's end, block 0, k 0).  In write mode, which starts from true states, the same
// events are the stream's errors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VUNET_SYNC_FN __host__ __device__ __forceinline__
#else
#define VUNET_SYNC_FN inline
#endif

namespace vunet_jpeg_sync {

constexpr int kLook = 9;

// one Huffman table as the host decoder builds it (jpeg_entropy.h's Huff, flattened)
struct Table {
  uint16_t look[1 << kLook];   // (length << 8) | symbol for codes of <= kLook bits, 0 otherwise
  int32_t maxcode[18];
  int32_t valoff[17];
  uint8_t symbols[256];
};

// one image's device row: at most two DC tables (t[0], t[1]) and two AC tables (t[2], t[3]), which component uses which, and the
// shape of its MCU.  Luma and chroma may share a table.  VUNET_JPEG_HUFFDEC_TAB_BYTES of include/vunet_jpeg_huffdec.h
struct Tables {
  Table t[4];
  int32_t dc[3], ac[3];         // component c decodes with t[dc[c]] and t[ac[c]]
  int32_t per_mcu, hv;          // blocks per MCU (1, 3, 4 or 6), luma blocks among them (1, 2 or 4)
  int32_t restart, reserved;    // MCUs per restart interval, 0 = none
};
static_assert(sizeof(Table) == 1420 && sizeof(Tables) == 5720, "the table row is part of the ABI");

struct State {
  uint32_t pos;   // bit position in the stuffed bytes
  uint32_t at;    // (block index within the MCU << 8) | k
};

VUNET_SYNC_FN bool same(State a, State b) { return a.pos == b.pos && a.at == b.at; }

// where block `ordinal` of an image (scan order) lies in its coefficients (vunet_jpeg.h's layout), in blocks
struct Grid {
  int32_t per_mcu, hs, vs, cols, bw0, n0, n1;   // cols: MCUs per row; n0, n1: blocks of the luma plane and of one chroma plane
};

VUNET_SYNC_FN int64_t block_index(const Grid& g, uint32_t ordinal) {
  const int32_t hv = g.hs * g.vs;
  const int32_t m = (int32_t)(ordinal / (uint32_t)g.per_mcu), r = (int32_t)(ordinal % (uint32_t)g.per_mcu);
  if (r < hv) return (int64_t)((m / g.cols) * g.vs + r / g.hs) * g.bw0 + (m % g.cols) * g.hs + r % g.hs;
  return (int64_t)g.n0 + (int64_t)(r - hv) * g.n1 + m;
}

struct Reader {
  const uint8_t* d;
  uint32_t begin, next, end;   // the segment's first byte; the next byte to load; the segment's end
  uint64_t cached;             // the aligned eight bytes around the last byte read ...
  uintptr_t cached_at;         // ... and their address (0: none)
  uint32_t fed;         // zero bytes fed past the end
  uint64_t acc;
  int n, zeros;         // bits in acc; how many of them were fed past the end
  uint32_t skipped;     // one bit per byte loaded, youngest lowest: a stuffed 00 was dropped behind it

  // byte i of the segment (begin <= i < end).  One aligned 8-byte load serves eight calls; a word that reaches outside the segment
  // is put together from the segment's own bytes, so nothing outside [begin, end) is ever touched
  VUNET_SYNC_FN uint32_t byte(uint32_t i) {
    const uintptr_t p = (uintptr_t)(d + i), at = p & ~(uintptr_t)7;
    if (at != cached_at) {
      cached_at = at;
      if (at >= (uintptr_t)(d + begin) && at + 8 <= (uintptr_t)(d + end)) {
        cached = *reinterpret_cast<const uint64_t*>(at);
      } else {
        cached = 0;
        for (int j = 0; j < 8; ++j)
          if (at + j >= (uintptr_t)(d + begin) && at + j < (uintptr_t)(d + end))
            cached |= (uint64_t)*reinterpret_cast<const uint8_t*>(at + j) << (8 * j);
      }
    }
    return (uint32_t)(cached >> (8 * (p & 7))) & 0xFFu;
  }
  VUNET_SYNC_FN void push() {
    uint32_t b = 0, s = 0;
    if (next < end) {
      b = byte(next++);
      if (b == 0xFF && next < end && byte(next) == 0) {
        ++next;
        s = 1;
      }
    } else {
      zeros += 8;
      ++fed;
    }
    acc = (acc << 8) | b;
    skipped = (skipped << 1) | s;
    n += 8;
  }
  VUNET_SYNC_FN void init(const uint8_t* bytes, uint32_t seg_begin, uint32_t seg_end, uint32_t pos) {
    d = bytes;
    begin = seg_begin;
    end = seg_end;
    cached = 0;
    cached_at = 0;
    fed = 0;
    acc = 0;
    n = 0;
    zeros = 0;
    skipped = 0;
    next = pos >> 3;
    if (next < seg_begin) next = seg_begin;
    const int bit = (int)(pos & 7);
    // a guess that rests on a stuffed byte (the first byte of a subsequence behind an FF) moves behind it
    if (bit == 0 && next > seg_begin && next < end && byte(next) == 0 && byte(next - 1) == 0xFF) ++next;
    if (bit) {
      push();
      n -= bit;   // (the bits in front stay in acc above n: peek masks them off)
    }
  }
  VUNET_SYNC_FN void fill() {
    while (n <= 56) push();
  }
  // the position of the next unread bit: every byte still (partly) in acc that had a 00 dropped has it between here and `next`
  VUNET_SYNC_FN uint32_t pos() const {
    const int m = (n + 7) >> 3;
    return ((next + fed) << 3) - (uint32_t)n - 8u * (uint32_t)__builtin_popcount(skipped & ((1u << m) - 1u));
  }
  VUNET_SYNC_FN int peek(int k) const { return (int)((acc >> (n - k)) & ((1ull << k) - 1ull)); }   // 1 <= k <= 32 <= n
  VUNET_SYNC_FN void skip(int k) { n -= k; }
  VUNET_SYNC_FN int get(int k) {
    if (k == 0) return 0;
    const int v = peek(k);
    n -= k;
    return v;
  }
  VUNET_SYNC_FN int real() const { return n - zeros; }   // bits left that the segment really holds (negative: overrun)
};

// one Huffman symbol, or -1 (no such code).  Needs n >= 17
VUNET_SYNC_FN int symbol(Reader& br, const Table& h) {
  const int e = h.look[br.peek(kLook)];
  if (e) {
    br.skip((e >> 8) & 15);
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

VUNET_SYNC_FN int extend(int v, int s) { return (s == 0 || v >= (1 << (s - 1))) ? v : v - (1 << s) + 1; }

enum Status : int32_t {
  kDone = 0,    // the walk reached the subsequence's end
  kStop = 1,    // the next symbol needs bits that the segment does not hold: the state is the one in front of it
  kLost = 2,    // no such code, a DC category above 15 or an index past 63
  kRange = 3,   // write mode: the next block's ordinal is outside [lo, hi): nothing more is stored
};

struct Result {
  State s;
  uint32_t blocks;   // blocks begun
  int32_t status;
  int32_t left;      // write mode: real bits left in the segment behind the state (at most 64 are counted)
};

// When an image is flagged, i.e. handed to the host decoder: the two rules below are the kernels' and the host check's alike.
//
// The write walk of one subsequence (`last`: the last of its segment; `tail`: its segment is the image's last) saw what the host
// decoder refuses: a lost walk from a true state; a block cut short by the segment's end; a block outside its segment's MCUs (behind
// the image's last MCU leftover data is tolerated, as on the host); a segment that ends inside a block (the host would read on into
// the marker); eight or more bits left in front of a restart marker (the host wants the marker right behind the padding).
VUNET_SYNC_FN bool write_refused(const Result& R, bool last, bool tail) {
  const bool inside = (R.s.at & 0xFF) != 0;
  if (R.status == kLost || (R.status == kStop && inside) || (R.status == kRange && !tail)) return true;
  if (last && !tail && R.left >= 8) return true;
  return last && R.status != kRange && inside;
}

// A segment began `total` blocks where its MCUs hold `seg_blocks`: fewer is short everywhere, more only in front of a restart marker
VUNET_SYNC_FN bool segment_short(uint32_t total, uint32_t seg_blocks, bool tail) { return tail ? total < seg_blocks : total != seg_blocks; }

// Walks [s.pos, end_bit) of the segment [seg_begin, seg_end) of `bytes`.  Write: block `ordinal` is the next to begin (the one
// the walk may enter in the middle of is ordinal - 1); blocks with lo <= ordinal < hi are stored at coef + 64 * block_index, each AC
// term at zz[k] and the DC DIFFERENCE at [0]; others end the walk (kRange).
template <bool Write>
VUNET_SYNC_FN Result walk(const uint8_t* bytes, uint32_t seg_begin, uint32_t seg_end, State s, uint32_t end_bit, const Tables& T,
                          const uint8_t* zz, int16_t* coef, const Grid& g, uint32_t ordinal, uint32_t lo, uint32_t hi) {
  Result R;
  R.blocks = 0;
  R.left = 0;
  R.status = kDone;
  const uint32_t per_mcu = (uint32_t)T.per_mcu, hv = (uint32_t)T.hv;
  uint32_t blk = s.at >> 8, k = s.at & 0xFF, pos = s.pos;
  const State lost = {end_bit, 0u};
  if (per_mcu < 1 || per_mcu > 6 || hv < 1 || hv > per_mcu || per_mcu - hv > 2 || blk >= per_mcu || k > 63 || end_bit > (seg_end << 3) ||
      pos < (seg_begin << 3)) {
    R.s = lost;
    R.status = kLost;
    return R;
  }
  Reader br;
  br.init(bytes, seg_begin, seg_end, pos);
  int16_t* out = nullptr;
  if (Write && k != 0) {
    if (ordinal == 0 || ordinal - 1 < lo || ordinal - 1 >= hi) {
      R.s = s;
      R.status = kRange;
      return R;
    }
    out = coef + 64 * block_index(g, ordinal - 1);
  }
  // every symbol takes at least one bit: the walk ends after at most as many symbols as it has bits
  uint32_t budget = pos < end_bit ? end_bit - pos : 0u;
  while (pos < end_bit && budget-- > 0u) {
    br.fill();
    const int real = br.real();
    const uint32_t c = blk < hv ? 0u : blk - hv + 1u;   // (<= 2: per_mcu - hv <= 2)
    if (k == 0) {
      const int sym = symbol(br, T.t[T.dc[c] & 3]);
      if (sym < 0 || sym > 15) {
        R.status = (sym < 0 ? real < 16 : br.real() < 0) ? kStop : kLost;
        break;
      }
      const int v = extend(br.get(sym), sym);
      if (br.real() < 0) {
        R.status = kStop;
        break;
      }
      if (Write) {
        if (ordinal < lo || ordinal >= hi) {
          R.status = kRange;
          break;
        }
        out = coef + 64 * block_index(g, ordinal);
        out[0] = (int16_t)v;
      }
      ++ordinal;
      ++R.blocks;
      k = 1;
    } else {
      const int rs = symbol(br, T.t[T.ac[c] & 3]);
      if (rs < 0) {
        R.status = real < 16 ? kStop : kLost;
        break;
      }
      const int r = rs >> 4, size = rs & 15;
      if (size == 0) {
        if (br.real() < 0) {
          R.status = kStop;
          break;
        }
        k = r == 15 ? k + 16 : 64;   // sixteen zeros, or the end of the block
      } else {
        const uint32_t at = k + (uint32_t)r;
        const int v = extend(br.get(size), size);
        if (br.real() < 0) {
          R.status = kStop;
          break;
        }
        if (at > 63) {
          R.status = kLost;
          break;
        }
        if (Write) out[zz[at]] = (int16_t)v;
        k = at + 1;
      }
      if (k >= 64) {   // (a run of sixteen zeros that passes 63 ends the block too, as on the host)
        k = 0;
        blk = blk + 1 == per_mcu ? 0 : blk + 1;
      }
    }
    pos = br.pos();
  }
  if (R.status == kLost) {
    R.s = lost;
    return R;
  }
  R.s.pos = pos;
  R.s.at = (blk << 8) | k;
  if (Write) {
    // what the host asks in front of a restart marker: fewer than eight bits of the segment are left
    Reader tail;
    tail.init(bytes, seg_begin, seg_end, pos);
    tail.fill();
    R.left = tail.real();
  }
  return R;
}

}  // namespace vunet_jpeg_sync
