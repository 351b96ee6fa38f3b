// A stand-alone harness for the device entropy decoder's walk (csrc/jpeg_sync.h is plain C++ under a host compiler): the rounds of
// csrc/jpeg_huff_dec.hip restated on the CPU -- marker scan, subsequence rows, Jacobi rounds of the kernel's own walk() until no
// exit state changes, the segmented prefix sum, the write pass, the DC sums -- and compared with the host decoder (entropy_decode).
// Neither HIP nor the library is involved.  Every stream given on the command line, every prefix of it and seeded single-bit flips
// inside its scan go through it at subsequence sizes 8, 16 and VUNET_JPEG_SUBSEQ_BYTES; the scan's bytes, the rows, the states and
// the coefficients each live in a heap buffer of exactly the announced size, so that a build with -fsanitize=address,undefined
// reports any access outside them.  The streams come from
//     python tests/golden/make_golden_jpeg.py --dump DIR
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_sync_check.cpp -o jpeg_sync_check
//     ./jpeg_sync_check DIR/*.jpg
//
// Checked: a clean stream is decoded without a flag to the host's coefficients; a damaged stream ends flagged (it would go to the
// host decoder), or unflagged and equal to what the host decoder accepts; the rounds never exceed the bound (the subsequences of
// the longest segment + 1: with one thread per "workgroup" that is the bound of the kernels).  Exits 1 otherwise.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../behavior_driven_video_synthesis_amd/csrc/jpeg_entropy.h"
#include "../behavior_driven_video_synthesis_amd/csrc/jpeg_sync.h"

namespace S = vunet_jpeg_sync;

static std::map<std::string, long> g_ends;
static long g_max_rounds = 0, g_fail = 0;

enum { kEqual = 0, kFlagged = 1, kIrregular = 2, kRefused = 3 };

// -> how the device route ends on d[0 .. len) at subsequence size `sub`; *coef: its coefficients where it ends unflagged
static int device_route(const uint8_t* d, int64_t len, int sub, const vunet_jpeg_info& info, int16_t* coef, long* rounds_out) {
  const int64_t expected = vunet_jpeg::expected_segments(info);
  std::vector<int64_t> segs((size_t)expected * 3);
  int64_t nseg = 0;
  uint16_t* qtab = new uint16_t[info.ncomp * 64];
  uint8_t* tab = new uint8_t[VUNET_JPEG_HUFFDEC_TAB_BYTES];
  const int rc = vunet_jpeg::scan_segments(d, len, &info, segs.data(), expected, &nseg, qtab, tab);
  S::Tables* T = new S::Tables();
  memcpy(T, tab, sizeof(*T));
  delete[] qtab;
  delete[] tab;
  if (rc != 0) {
    delete T;
    return rc == VUNET_JPEG_HUFFDEC_IRREGULAR ? kIrregular : kRefused;
  }
  // the scan's bytes alone, in a buffer of exactly their size
  const int64_t lo = segs[0], hi = segs[3 * (nseg - 1) + 1];
  uint8_t* bytes = new uint8_t[hi - lo];
  memcpy(bytes, d + lo, (size_t)(hi - lo));
  int64_t want = 0, longest = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t n = (segs[3 * s + 1] - segs[3 * s] + sub - 1) / sub;
    want += n;
    longest = n > longest ? n : longest;
  }
  const int64_t cap = (want + VUNET_JPEG_HUFFDEC_GROUP - 1) / VUNET_JPEG_HUFFDEC_GROUP * VUNET_JPEG_HUFFDEC_GROUP;
  vunet_jpeg_subseq* rows = new vunet_jpeg_subseq[cap];
  int64_t nrows = 0;
  int end = kFlagged;
  vunet_jpeg_img img;
  memset(&img, 0, sizeof(img));
  img.height = info.height, img.width = info.width, img.ncomp = info.ncomp, img.hsamp = info.hsamp, img.vsamp = info.vsamp;
  img.bw0 = info.bw0, img.bh0 = info.bh0, img.bw1 = info.bw1, img.bh1 = info.bh1;
  if (vunet_jpeg::subseq_rows(segs.data(), nseg, &info, 0, -lo, 0, rows, cap, &nrows, sub) != 0 || nrows != cap ||
      !vunet_jpeg::subseq_rows_ok(rows, nrows, hi - lo, &img, 1, sub) || !vunet_jpeg::table_rows_ok((const uint8_t*)T, &img, 1)) {
    fprintf(stderr, "rows refused (%lld segments, %lld rows)\n", (long long)nseg, (long long)want);
    ++g_fail;
  } else {
    // Jacobi rounds, one "thread" per row
    S::State* exits = new S::State[want];
    S::State* next = new S::State[want];
    S::State* walked = new S::State[want];
    uint32_t* begun = new uint32_t[want];
    for (int64_t i = 0; i < want; ++i) {
      exits[i] = S::State{(uint32_t)rows[i].end << 3, 0u};
      walked[i] = S::State{0xFFFFFFFFu, 0xFFFFFFFFu};
      begun[i] = 0;
    }
    const S::Grid none = {1, 1, 1, 1, 1, 0, 0};
    long rounds = 0;
    for (;;) {
      ++rounds;
      long moved = 0;
      for (int64_t i = 0; i < want; ++i) {
        const vunet_jpeg_subseq& r = rows[i];
        const S::State entry = (r.flags & VUNET_JPEG_SUBSEQ_FIRST) ? S::State{(uint32_t)r.begin << 3, 0u} : exits[i - 1];
        next[i] = exits[i];
        if (S::same(entry, walked[i])) continue;
        const S::Result R = S::walk<false>(bytes, (uint32_t)r.seg_begin, (uint32_t)r.seg_end, entry, (uint32_t)r.end << 3, *T,
                                           vunet_jpeg::kZigzag, nullptr, none, 0u, 0u, 0u);
        walked[i] = entry;
        begun[i] = R.blocks;
        moved += !S::same(R.s, exits[i]);
        next[i] = R.s;
      }
      S::State* t = exits;
      exits = next;
      next = t;
      if (moved == 0 || rounds > longest + 1) break;
    }
    if (rounds > longest + 1) {
      fprintf(stderr, "%ld rounds for %lld subsequences in the longest segment\n", rounds, (long long)longest);
      ++g_fail;
    }
    g_max_rounds = rounds > g_max_rounds ? rounds : g_max_rounds;
    *rounds_out = rounds;
    // block ordinals and the write pass
    uint32_t flags = 0;
    std::vector<uint32_t> ordinal((size_t)want);
    uint32_t in_seg = 0;
    for (int64_t i = 0; i < want; ++i) {
      const vunet_jpeg_subseq& r = rows[i];
      if (r.flags & VUNET_JPEG_SUBSEQ_FIRST) in_seg = 0;
      ordinal[(size_t)i] = (uint32_t)r.first_block + in_seg;
      in_seg += begun[i];
      if ((r.flags & VUNET_JPEG_SUBSEQ_LAST) && S::segment_short(in_seg, (uint32_t)r.seg_blocks, (r.flags & VUNET_JPEG_SUBSEQ_TAIL) != 0))
        flags |= VUNET_JPEG_HUFFDEC_SHORT;
    }
    memset(coef, 0, (size_t)info.ncoef * sizeof(int16_t));
    const S::Grid g = {T->per_mcu, info.hsamp, info.vsamp, info.bw0 / info.hsamp, info.bw0, info.bw0 * info.bh0, info.bw1 * info.bh1};
    for (int64_t i = 0; i < want; ++i) {
      const vunet_jpeg_subseq& r = rows[i];
      const bool tail = r.flags & VUNET_JPEG_SUBSEQ_TAIL;
      const S::State entry = (r.flags & VUNET_JPEG_SUBSEQ_FIRST) ? S::State{(uint32_t)r.begin << 3, 0u} : exits[i - 1];
      uint32_t top = (uint32_t)r.first_block + (uint32_t)r.seg_blocks;
      top = top < (uint32_t)info.nblocks ? top : (uint32_t)info.nblocks;
      const S::Result R = S::walk<true>(bytes, (uint32_t)r.seg_begin, (uint32_t)r.seg_end, entry, (uint32_t)r.end << 3, *T,
                                        vunet_jpeg::kZigzag, coef, g, ordinal[(size_t)i], (uint32_t)r.first_block, top);
      if (S::write_refused(R, (r.flags & VUNET_JPEG_SUBSEQ_LAST) != 0, tail)) flags |= VUNET_JPEG_HUFFDEC_ERROR;
    }
    // the DC sums per component in scan order, reset at every restart interval
    const int hv = T->hv, per = T->per_mcu;
    uint32_t pred[3] = {0, 0, 0};
    for (int32_t b = 0; b < info.nblocks; ++b) {
      const int m = b / per, r = b % per, c = r < hv ? 0 : r - hv + 1;
      if (info.restart > 0 && r == 0 && m % info.restart == 0) pred[0] = pred[1] = pred[2] = 0;
      int16_t* blk = coef + 64 * S::block_index(g, (uint32_t)b);
      pred[c] += (uint32_t)(int32_t)blk[0];
      blk[0] = (int16_t)(uint16_t)pred[c];
    }
    end = flags ? kFlagged : kEqual;
    delete[] exits;
    delete[] next;
    delete[] walked;
    delete[] begun;
  }
  delete[] rows;
  delete[] bytes;
  delete T;
  return end;
}

// d[0 .. len) through both decoders at every subsequence size.  clean: a whole supported stream
static void run(const uint8_t* src, size_t len, bool clean, const char* what) {
  uint8_t* d = new uint8_t[len ? len : 1];   // exactly len bytes: one byte too many read is a report
  memcpy(d, src, len);
  vunet_jpeg_info info;
  int rc = vunet_jpeg::parse_info(d, (int64_t)len, &info);
  if (rc != 0) {
    ++g_ends["refused by the header parse"];
    if (clean) {
      fprintf(stderr, "%s: header code %d\n", what, rc);
      ++g_fail;
    }
    delete[] d;
    return;
  }
  int16_t* host = new int16_t[info.ncoef];
  int16_t* dev = new int16_t[info.ncoef];
  uint16_t* qtab = new uint16_t[info.ncomp * 64];
  rc = vunet_jpeg::entropy_decode(d, (int64_t)len, &info, host, qtab);
  const int sizes[3] = {8, 16, VUNET_JPEG_SUBSEQ_BYTES};
  for (int s = 0; s < 3; ++s) {
    long rounds = 0;
    const int end = device_route(d, (int64_t)len, sizes[s], info, dev, &rounds);
    const bool equal = end == kEqual && rc == 0 && memcmp(host, dev, (size_t)info.ncoef * sizeof(int16_t)) == 0;
    if (end == kEqual && !equal) {
      fprintf(stderr, "%s (%zu bytes, subsequences of %d): unflagged, but the host decoder %s\n", what, len, sizes[s],
              rc ? "refuses the stream" : "gives other coefficients");
      ++g_fail;
    } else if (clean && end != kEqual) {
      fprintf(stderr, "%s (subsequences of %d): a clean stream ended %d\n", what, sizes[s], end);
      ++g_fail;
    }
    ++g_ends[end == kEqual ? "decoded, equal to the host decoder" : end == kFlagged ? (rc ? "flagged, the host decoder refuses it" : "flagged, the host decoder accepts it")
                           : end == kIrregular ? (rc ? "irregular, the host decoder refuses it" : "irregular, the host decoder accepts it")
                                               : "refused by the header parse"];
  }
  delete[] host;
  delete[] dev;
  delete[] qtab;
  delete[] d;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]);
    return 2;
  }
  long inputs = 0;
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    std::vector<uint8_t> data;
    uint8_t chunk[4096];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) data.insert(data.end(), chunk, chunk + n);
    fclose(f);
    if (std::string(argv[a]).find("refused_") != std::string::npos) continue;   // (outside the supported subset: the header parse's)
    run(data.data(), data.size(), true, argv[a]);
    for (size_t len = 0; len < data.size(); ++len) run(data.data(), len, false, argv[a]);   // every truncation
    // seeded single-bit flips inside the scan
    vunet_jpeg::Header* H = new vunet_jpeg::Header();
    const int64_t scan = vunet_jpeg::parse(data.data(), (int64_t)data.size(), *H) == 0 ? H->scan : 0;
    delete H;
    std::vector<uint8_t> flip(data);
    const size_t span = data.size() - (size_t)scan, flips = span < 256 ? span : 256;
    for (size_t i = 0; i < flips; ++i) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      const size_t at = (size_t)scan + (size_t)((seed >> 33) % span);
      flip[at] ^= (uint8_t)(1u << ((seed >> 29) & 7));
      const std::string label = std::string(argv[a]) + ": bit " + std::to_string((seed >> 29) & 7) + " of byte " + std::to_string(at) + " flipped";
      run(flip.data(), flip.size(), false, label.c_str());
      flip[at] = data[at];
    }
    inputs += 1 + (long)data.size() + (long)flips;
  }
  printf("%ld inputs from %d streams, each at subsequences of 8, 16 and %d bytes; at most %ld rounds\n", inputs, argc - 1,
         VUNET_JPEG_SUBSEQ_BYTES, g_max_rounds);
  for (const auto& kv : g_ends) printf("  %-45s %ld\n", kv.first.c_str(), kv.second);
  if (g_fail) printf("%ld FAILURES\n", g_fail);
  return g_fail ? 1 : 0;
}
