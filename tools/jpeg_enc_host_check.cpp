// A stand-alone harness for the host half of the JPEG encoder (csrc/jpeg_huff_enc.h has no HIP in it): seeded coefficient sets of
// every sampling, from sparse to every term at its largest, go through entropy_encode into heap buffers of EXACTLY `cap` bytes, for
// cap = the bound, the stream's own length, every shorter capacity of the small sets and a spread of them for the rest -- so that
// a build with -fsanitize=address,undefined reports any write at or past out + cap and any read outside the coefficients.  Each
// whole stream is decoded again with csrc/jpeg_entropy.h and compared with what went in; out-of-range terms must be refused.
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_enc_host_check.cpp -o jpeg_enc_host_check
//     ./jpeg_enc_host_check
//
// Prints how many calls ended in each return code; exits 1 on any mismatch.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "../behavior_driven_video_synthesis_amd/csrc/jpeg_huff_enc.h"

static std::map<int, long> g_codes;
static uint64_t g_state = 0x9E3779B97F4A7C15ull;

static uint32_t rnd() {   // xorshift64*
  g_state ^= g_state >> 12;
  g_state ^= g_state << 25;
  g_state ^= g_state >> 27;
  return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}

// -> the return code; *len as the library left it; `got` the cap bytes
static int run(const std::vector<int16_t>& coef, const vunet_jpeg_info& info, const uint16_t* qtab, int64_t cap, int64_t* len,
               std::vector<uint8_t>* got) {
  int16_t* c = new int16_t[coef.size()];   // exactly ncoef coefficients and cap bytes: one too many touched is a report
  memcpy(c, coef.data(), coef.size() * sizeof(int16_t));
  uint8_t* out = new uint8_t[cap ? cap : 1];
  const int rc = vunet_jpeg::entropy_encode(c, &info, qtab, out, cap, len);
  if (got) got->assign(out, out + cap);
  delete[] out;
  delete[] c;
  ++g_codes[rc];
  return rc;
}

int main() {
  const int shapes[][5] = {{1, 1, 3, 2, 2},  {8, 8, 3, 2, 2},   {17, 23, 3, 2, 2}, {17, 23, 3, 2, 1}, {17, 23, 3, 1, 1}, {24, 8, 3, 2, 2},
                           {8, 24, 3, 2, 2}, {250, 1, 3, 2, 1}, {1, 250, 3, 2, 2}, {37, 45, 1, 1, 1}, {64, 64, 3, 2, 2}, {40, 72, 3, 1, 1}};
  int bad = 0;
  long sets = 0;
  for (const auto& s : shapes) {
    vunet_jpeg_info info;
    if (vunet_jpeg::encode_info(s[0], s[1], s[2], s[3], s[4], &info) != 0) return 2;
    int64_t bound = 0;
    if (vunet_jpeg::encode_bound(&info, &bound) != 0) return 2;
    for (int fill = 0; fill < 6; ++fill, ++sets) {
      uint16_t qtab[192];
      vunet_jpeg::quant_tables(fill == 0 ? 30 : (fill == 1 ? 75 : 100), qtab);
      memcpy(qtab + 128, qtab + 64, 128);
      std::vector<int16_t> coef((size_t)info.ncoef);
      for (size_t i = 0; i < coef.size(); ++i) {
        const bool is_dc = i % 64 == 0;
        int v = 0;
        if (fill == 0) v = rnd() % 16 == 0 ? (int)(rnd() % 31) - 15 : 0;                       // sparse: runs, ZRL, EOB
        else if (fill == 1) v = rnd() % 3 == 0 ? (int)(rnd() % 255) - 127 : 0;
        else if (fill == 2) v = (int)(rnd() % 2047) - 1023;                                    // dense, the whole AC range
        else if (fill == 3) v = (rnd() & 1) ? 1023 : -1023;                                    // the longest codes
        else if (fill == 4) v = i % 64 == 63 ? 1 : 0;                                          // three ZRLs per block
        else v = -1;                                                                           // bytes of 1-bits: stuffing
        if (is_dc && fill >= 2 && fill <= 3) v = (int)(rnd() % 2047) - 1023;                   // differences of up to 11 bits
        coef[i] = (int16_t)v;
      }
      int64_t len = -1;
      std::vector<uint8_t> whole;
      if (run(coef, info, qtab, bound, &len, &whole) != 0 || len < 4 || len > bound) {
        fprintf(stderr, "%dx%d fill %d: the bound did not hold (len %lld)\n", s[0], s[1], fill, (long long)len);
        return 1;
      }
      whole.resize((size_t)len);
      // the decoder gives back what went in
      vunet_jpeg_info back;
      std::vector<int16_t> dec((size_t)info.ncoef);
      uint16_t q2[192];
      if (vunet_jpeg::parse_info(whole.data(), len, &back) != 0 || !vunet_jpeg::same_info(back, info) ||
          vunet_jpeg::entropy_decode(whole.data(), len, &back, dec.data(), q2) != 0 || dec != coef ||
          memcmp(q2, qtab, 128 * (size_t)info.ncomp) != 0) {
        fprintf(stderr, "%dx%d fill %d: the stream does not decode to its coefficients\n", s[0], s[1], fill);
        bad = 1;
      }
      // capacities: exact, and short ones -- all of them for the small sets, a spread for the rest
      const int64_t step = len <= 1500 ? 1 : len / 97 + 1;
      std::vector<uint8_t> got;
      for (int64_t cap = len; cap >= 0; cap = (cap == len ? len - 1 : cap - step)) {
        int64_t need = -1;
        const int rc = run(coef, info, qtab, cap, &need, &got);
        const int want = cap == len ? 0 : VUNET_JPEG_ERR_CAPACITY;
        if (rc != want || need != len || memcmp(got.data(), whole.data(), (size_t)cap) != 0) {
          fprintf(stderr, "%dx%d fill %d cap %lld: code %d, length %lld\n", s[0], s[1], fill, (long long)cap, rc, (long long)need);
          bad = 1;
        }
      }
      // one term outside baseline's range anywhere in the set is refused
      for (int k = 0; k < 4; ++k) {
        std::vector<int16_t> c2(coef);
        const size_t at = rnd() % c2.size();
        c2[at] = (int16_t)((at % 64 == 0) ? ((k & 1) ? 4095 : -4095) : ((k & 1) ? 1024 : -32768));
        int64_t need = -1;
        if (run(c2, info, qtab, bound, &need, nullptr) != VUNET_JPEG_ERR_RANGE || need != 0) {
          fprintf(stderr, "%dx%d fill %d: coefficient %d at %zu was not refused\n", s[0], s[1], fill, (int)c2[at], at);
          bad = 1;
        }
      }
    }
  }
  printf("%ld coefficient sets\n", sets);
  for (const auto& kv : g_codes) printf("  code %4d: %ld\n", kv.first, kv.second);
  return bad;
}
