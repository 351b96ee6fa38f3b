/*
 * skeleton_ref.c -- sequential reference of the skeleton canvas (TEST INFRASTRUCTURE ONLY): add_joints_to_img
 * (lib/utils.py:733-750) on a canvas filled with the background colour, through the drawing primitives of
 * oracle/stickman_oracle.c, which is included unchanged.  Per frame: three planes filled with `background`, then for each
 * limb in list order and each plane the oracle's own draw_thick_line with that plane's colour byte.  End points are
 * truncated toward zero as Python's int() does; there is no validity rule.
 */
#include "../oracle/stickman_oracle.c"

/* kps [F][J][2] float (x, y); limbs [L][2]; colors [L][3]; out [F][3][H][W] uint8 */
void skeleton_ref_draw(const float* kps, int F, int J, const int32_t* limbs, const uint8_t* colors, int L, uint8_t* out,
                       int H, int W, int thickness, int background) {
  memset(out, background, (size_t)F * 3 * H * W);
  for (int f = 0; f < F; ++f) {
    const float* k = kps + (size_t)f * J * 2;
    for (int c = 0; c < L; ++c) {
      const int a = limbs[2 * c], b = limbs[2 * c + 1];
      for (int p = 0; p < 3; ++p)
        draw_thick_line(out + ((size_t)f * 3 + p) * H * W, W, H, (int64_t)k[2 * a], (int64_t)k[2 * a + 1], (int64_t)k[2 * b],
                        (int64_t)k[2 * b + 1], colors[3 * c + p], thickness);
    }
  }
}
