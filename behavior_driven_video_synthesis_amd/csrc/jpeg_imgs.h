// The host-side check of the vunet_jpeg_img rows that the JPEG decoder (jpeg.hip) and encoder (jpeg_enc.hip) share: both hand the
// host copy of their descriptors to it before anything is launched.  Plain C++, no HIP.
#pragma once
#include <stdint.h>

#include "../../include/vunet_jpeg.h"

namespace vunet_jpeg {

// every row of the host copy of the descriptors against the buffers: nothing is launched on a row that could index outside them
inline bool imgs_ok(const vunet_jpeg_img* h, int N, int64_t coef_count, int64_t qtab_count, int64_t planes_bytes, int Hmax, int Wmax,
                    int slots, int64_t* total) {
  int64_t blocks = 0;
  for (int n = 0; n < N; ++n) {
    const vunet_jpeg_img& m = h[n];
    const bool s = (m.hsamp == 1 && m.vsamp == 1) || (m.ncomp == 3 && m.hsamp == 2 && (m.vsamp == 1 || m.vsamp == 2));
    if (!s || (m.ncomp != 1 && m.ncomp != 3) || m.height < 1 || m.width < 1 || m.height > Hmax || m.width > Wmax) return false;
    if (m.bw0 < (m.width + 7) / 8 || m.bh0 < (m.height + 7) / 8 || m.bw0 > 8192 || m.bh0 > 8192) return false;
    if (m.ncomp == 3) {
      const int cw = (m.width + m.hsamp - 1) / m.hsamp, ch = (m.height + m.vsamp - 1) / m.vsamp;
      if (m.bw1 < (cw + 7) / 8 || m.bh1 < (ch + 7) / 8 || m.bw1 > 8192 || m.bh1 > 8192) return false;
    } else if (m.bw1 != 0 || m.bh1 != 0) {
      return false;
    }
    const int64_t nb = (int64_t)m.bw0 * m.bh0 + 2 * (int64_t)m.bw1 * m.bh1;
    if (m.block0 != blocks || m.slot < 0 || m.slot >= slots) return false;
    blocks += nb;
    if (blocks > 0x7FFFFFFF) return false;
    if (m.coef_off < 0 || m.coef_off % 64 || m.coef_off > coef_count - nb * 64) return false;
    if (m.q_off < 0 || m.q_off % 8 || m.q_off > qtab_count - m.ncomp * 64) return false;
    if (m.plane_off < 0 || m.plane_off % 16 || m.plane_off > planes_bytes - nb * 64) return false;
  }
  *total = blocks;
  return true;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace vunet_jpeg
