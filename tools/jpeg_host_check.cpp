// A stand-alone harness for the host half of the JPEG decoder (csrc/jpeg_entropy.h has no HIP in it): every stream given on the
// command line, every prefix of it and one flipped bit per byte of it go through parse + entropy_decode, each from a heap copy of
// exactly its length and into buffers of exactly the announced sizes -- so that a build with -fsanitize=address,undefined reports
// any read past `len` or write past ncoef / ncomp * 64.  The streams come from
//     python tests/golden/make_golden_jpeg.py --dump DIR
//
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//     ./jpeg_host_check DIR/*.jpg
//
// Prints how many inputs ended in each return code; exits 1 if a whole supported stream did not decode.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../behavior_driven_video_synthesis_amd/csrc/jpeg_entropy.h"

static std::map<int, long> g_codes;

// -> the return code of parse, or of entropy_decode where the parse succeeded
static int run(const uint8_t* src, size_t len) {
  uint8_t* d = new uint8_t[len ? len : 1];   // exactly len bytes: one byte too many read is a report
  memcpy(d, src, len);
  vunet_jpeg_info info;
  int rc = vunet_jpeg::parse_info(d, (int64_t)len, &info);
  if (rc == 0) {
    int16_t* coef = new int16_t[info.ncoef];
    uint16_t* qtab = new uint16_t[info.ncomp * 64];
    rc = vunet_jpeg::entropy_decode(d, (int64_t)len, &info, coef, qtab);
    delete[] coef;
    delete[] qtab;
  }
  delete[] d;
  ++g_codes[rc];
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s stream.jpg ...\n", argv[0]);
    return 2;
  }
  int bad = 0;
  long inputs = 0;
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
    const int whole = run(data.data(), data.size());
    const bool refused = std::string(argv[a]).find("refused_") != std::string::npos;
    if (refused ? !(whole <= -110 && whole >= -119) : whole != 0) {
      fprintf(stderr, "%s: code %d\n", argv[a], whole);
      bad = 1;
    }
    for (size_t len = 0; len < data.size(); ++len) run(data.data(), len);   // every truncation
    std::vector<uint8_t> flip(data);
    for (size_t i = 0; i < data.size(); ++i) {                             // one flipped bit per byte, headers included
      flip[i] ^= (uint8_t)(1u << (i % 8));
      run(flip.data(), flip.size());
      flip[i] = data[i];
    }
    inputs += 1 + 2 * (long)data.size();
  }
  printf("%ld inputs from %d streams\n", inputs, argc - 1);
  for (const auto& kv : g_codes) printf("  code %4d: %ld\n", kv.first, kv.second);
  return bad;
}
