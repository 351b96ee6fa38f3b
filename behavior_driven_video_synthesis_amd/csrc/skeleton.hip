// Skeleton frames of the pose-only videos on the GPU (data/data_conversions_3d.py:1068-1228 project_onto_image_plane;
// lib/utils.py:733-750 add_joints_to_img): every limb a cv2.line of one colour on a canvas of the camera's image size, the
// canvas resized with INTER_NEAREST, optionally cut to a person-centred strip and laid over a synthesised frame.
//
// The canvas is never built.  The closed forms of raster_forms.h answer "does limb c cover canvas pixel (x, y)?" for any
// pixel, so a lane evaluates them only at the canvas pixels that nearest-neighbour sampling keeps: output pixel (y, x) is
// canvas pixel (sy[y], sx[x + crop offset]).  A workgroup serves one frame: its prologue reduces the limbs to integer
// parameters in LDS (one lane per limb; lane 255 the two crop offsets in float64, lane 254 the circle table), then it walks
// 16 x 64 output tiles, each lane owning four adjacent pixels of one row and each wavefront a 4 x 64 patch.  Per patch a
// first pass without a branch votes every limb's padded bounding box against the lanes' sampled coordinates into one
// wave-uniform bit mask (so the LDS reads of all limbs are in flight together; the vote is taken on the coordinates
// themselves and holds for any table, monotone or not).  Only the limbs of that mask are looked at again: a pixel is a
// candidate if it also lies within the limb's padded half width of the line through its end points (one float64 cross
// product, exact for these integers), and the closed forms run on candidates only, skipped wave-uniformly where a
// wavefront has none.  Both tests are supersets of what OpenCV draws; they never decide a colour.  Colours are
// kept as one packed 24-bit value per pixel (the last limb that covers a pixel gives it all three channels); four pixels
// leave as three dwords where the address is dword-aligned and the row has all four, as bytes otherwise.
// No memory access depends on a table value or a keypoint: the only data-dependent indices are joint numbers, and a limb
// or crop joint outside [0, J) is dropped.  Bit-exact against the sequential restatement in oracle/stickman_oracle.c.
#include "common.h"
#include "raster_forms.h"
#include "../../include/vunet_skeleton.h"

#define SK_MAXLIMB VUNET_SKELETON_MAX_LIMBS
#define SK_TILE_H 16
#define SK_TILE_W 64

struct SkArgs {
  const float* kps;
  const int* limbs;
  const uint8_t* colors;
  const int* sy;
  const int* sx;
  const int* crop_joints;
  const uint8_t* rgb;
  uint8_t* out_skel;
  uint8_t* out_overlay;
  uint8_t* out_rgb;
  int* span;
  long long skel_fs, skel_rs;
  double skel_div, rgb_mul;
  int J, L, Hs, Ws, thickness, background, Ht, Wt, tw, n_crop, Sw;
};

struct __attribute__((aligned(4))) SkDw3 {
  uint32_t a, b, c;
};

// four channels-last pixels (24-bit packed colours) to p: three dwords, or the first n pixels as bytes
__device__ __forceinline__ void sk_store4(uint8_t* p, const uint32_t* col, int n) {
  if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
    SkDw3 v;
    v.a = col[0] | (col[1] << 24);
    v.b = (col[1] >> 8) | (col[2] << 16);
    v.c = (col[2] >> 16) | (col[3] << 8);
    *reinterpret_cast<SkDw3*>(p) = v;
  } else {
    for (int i = 0; i < n; ++i) {
      p[3 * i] = (uint8_t)(col[i] & 255u);
      p[3 * i + 1] = (uint8_t)((col[i] >> 8) & 255u);
      p[3 * i + 2] = (uint8_t)((col[i] >> 16) & 255u);
    }
  }
}

// int(min(max(0, centre - tw // 2), bound)) of :1181-1182 / :1198-1199, centre = (sum of the joints' scaled x) / n
__device__ __forceinline__ int sk_strip_start(double sum, int n, int tw, int bound) {
  double v = __dsub_rn(__ddiv_rn(sum, (double)n), (double)(tw / 2));
  if (!(v > 0.0)) v = 0.0;
  if ((double)bound < v) v = (double)bound;
  return (int)v;
}

__global__ __launch_bounds__(256) void skeleton_raster_kernel(const SkArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char thick_raw[];   // RThick[L] when thickness > 1
  RThick* const thick = reinterpret_cast<RThick*>(thick_raw);
  __shared__ RLine lines[SK_MAXLIMB];
  __shared__ int bx0[SK_MAXLIMB], bx1[SK_MAXLIMB], by0[SK_MAXLIMB], by1[SK_MAXLIMB];   // padded boxes, canvas pixels
  __shared__ uint32_t lcol[SK_MAXLIMB];
  __shared__ double lax[SK_MAXLIMB], lay[SK_MAXLIMB], ldx[SK_MAXLIMB], ldy[SK_MAXLIMB], lthr[SK_MAXLIMB];   // the strip test
  __shared__ int chw[R_MAXRAD + 1];
  __shared__ int off[2];   // first column of the skeleton strip / of the rgb strip
  const int f = blockIdx.x, tid = threadIdx.x;
  const float* k = a.kps + (size_t)f * a.J * 2;
  const bool is_thick = a.thickness > 1;
  const int radius = is_thick ? ((a.thickness << (XY_SHIFT - 1)) + (XY_ONE >> 1)) >> XY_SHIFT : 0;

  if (tid < a.L) {
    const int ja = a.limbs[2 * tid], jb = a.limbs[2 * tid + 1];
    RLine ln;
    ln.valid = 0;
    int x0 = 1, x1 = 0, y0 = 1, y1 = 0;   // an empty box: the limb is never evaluated
    if (ja >= 0 && ja < a.J && jb >= 0 && jb < a.J) {
      // int(): truncation toward zero, negative coordinates included (no validity rule here, unlike make_joint_img)
      const long long ax = (long long)k[2 * ja], ay = (long long)k[2 * ja + 1];
      const long long bx = (long long)k[2 * jb], by = (long long)k[2 * jb + 1];
      // the quad's corners lie within (thickness + 1) / 2 of an end point, the caps within the radius; + 2 for the roundings
      const long long pad = is_thick ? (a.thickness + 1) / 2 + 2 : 1;
      const long long lx0 = min(ax, bx) - pad, lx1 = max(ax, bx) + pad, ly0 = min(ay, by) - pad, ly1 = max(ay, by) + pad;
      // A limb whose padded box misses the canvas draws nothing and is dropped here, exactly.  One with an end point
      // beyond +-2^20 pixels is dropped too (VUNET_SKELETON_COORD_LIMIT): FillConvexPoly's chain walk takes one step
      // per row between the quad's top and the canvas, and that bounds the prologue's run time.
      const long long lim = VUNET_SKELETON_COORD_LIMIT;
      const bool far = ax < -lim || ax > lim || ay < -lim || ay > lim || bx < -lim || bx > lim || by < -lim || by > lim;
      if (!far && lx1 >= 0 && ly1 >= 0 && lx0 < a.Ws && ly0 < a.Hs) {
        if (is_thick) r_make_thick(thick[tid], ax, ay, bx, by, a.thickness, a.Ws, a.Hs);
        else ln = r_make_line(ax, ay, bx, by, a.Ws, a.Hs);
        x0 = (int)lx0;
        x1 = (int)lx1;
        y0 = (int)ly0;
        y1 = (int)ly1;
        // Every pixel OpenCV sets lies within `half` of the line through the end points: the quad's half width
        // (thickness + 1) / 2 or the cap radius (thin: the clip moves an end point by < 1, the iterator strays by 1/2), pixel
        // and vertex roundings (< 1.5), and the drift of the fixed-point walks -- FillConvexPoly's edge chains and Line2 lose
        // < 2^-16 pixel per row or step, over at most `reach` of them.  |cross| <= half * length is that distance test.
        const long long reach = max(max(max(ax < 0 ? -ax : ax, bx < 0 ? -bx : bx), max(ay < 0 ? -ay : ay, by < 0 ? -by : by)),
                                    (long long)max(a.Ws, a.Hs));
        const double half = (is_thick ? 0.5 * (double)(a.thickness + 1) : 1.5) + 2.0 + (double)reach * (1.0 / 32768.0);
        const double ddx = (double)(bx - ax), ddy = (double)(by - ay);
        lax[tid] = (double)ax;
        lay[tid] = (double)ay;
        ldx[tid] = ddx;
        ldy[tid] = ddy;
        lthr[tid] = half * (sqrt(ddx * ddx + ddy * ddy) + 1.0);
      }
    }
    lines[tid] = ln;
    bx0[tid] = x0;
    bx1[tid] = x1;
    by0[tid] = y0;
    by1[tid] = y1;
    lcol[tid] = (uint32_t)a.colors[3 * tid] | ((uint32_t)a.colors[3 * tid + 1] << 8) | ((uint32_t)a.colors[3 * tid + 2] << 16);
  }
  if (tid == 254 && is_thick) r_circle_table(chw, radius);
  if (tid == 255) {
    int o0 = 0, o1 = 0;
    if (a.tw > 0) {
      // np.mean(kps / scaling, axis=0)[0] and np.mean(kps * joint_scaling, axis=0)[0]: float64, joints added in index order
      double s0 = 0.0, s1 = 0.0;
      const int n = a.crop_joints ? a.n_crop : a.J;
      for (int i = 0; i < n; ++i) {
        const int j = a.crop_joints ? a.crop_joints[i] : i;
        const double x = (j >= 0 && j < a.J) ? (double)k[2 * j] : 0.0;
        s0 = __dadd_rn(s0, __ddiv_rn(x, a.skel_div));
        s1 = __dadd_rn(s1, __dmul_rn(x, a.rgb_mul));
      }
      o0 = sk_strip_start(s0, n, a.tw, a.Wt - a.tw);
      if (a.Sw >= a.tw) o1 = sk_strip_start(s1, n, a.tw, a.Sw - a.tw);
      if (a.span && blockIdx.y == 0) {
        int* s = a.span + 4 * (size_t)f;
        s[0] = o0;
        s[1] = o0 + a.tw;
        s[2] = a.Sw >= a.tw ? o1 : 0;
        s[3] = a.Sw >= a.tw ? o1 + a.tw : 0;
      }
    }
    off[0] = o0;
    off[1] = o1;
  }
  __syncthreads();

  const int Wo = a.tw > 0 ? a.tw : a.Wt;
  const int o0 = off[0], o1 = off[1];
  const uint32_t bg = (uint32_t)a.background * 0x010101u;
  const int ntx = (Wo + SK_TILE_W - 1) / SK_TILE_W, nty = (a.Ht + SK_TILE_H - 1) / SK_TILE_H;
  for (int t = blockIdx.y; t < ntx * nty; t += gridDim.y) {
    const int ty = t / ntx, tx = t - ty * ntx;
    const int y = ty * SK_TILE_H + (tid >> 4), x0 = tx * SK_TILE_W + (tid & 15) * 4;
    const int n = (y < a.Ht && x0 < Wo) ? min(4, Wo - x0) : 0;   // this lane's pixels
    int cy = 0, cx[4] = {0, 0, 0, 0}, xmin = 0, xmax = 0;
    if (n > 0) {
      cy = a.sy ? a.sy[y] : y;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int xo = min(x0 + i, Wo - 1) + o0;   // (a lane's missing pixels repeat its last one; they are not stored)
        cx[i] = a.sx ? a.sx[xo] : xo;
      }
      xmin = min(min(cx[0], cx[1]), min(cx[2], cx[3]));
      xmax = max(max(cx[0], cx[1]), max(cx[2], cx[3]));
    }
    uint32_t col[4] = {bg, bg, bg, bg};
    unsigned long long todo = 0;   // wave-uniform: the limbs whose box holds a sampled pixel of this wavefront's patch
    for (int c = 0; c < a.L; ++c) {
      const bool in_box = n > 0 && cy >= by0[c] && cy <= by1[c] && xmax >= bx0[c] && xmin <= bx1[c];
      todo |= (unsigned long long)(__ballot(in_box) != 0) << c;
    }
    while (todo) {   // in list order: the later limb overwrites
      const int c = __builtin_ctzll(todo);
      todo &= todo - 1;
      unsigned cand = 0;
      if (n > 0 && cy >= by0[c] && cy <= by1[c] && xmax >= bx0[c] && xmin <= bx1[c]) {
        const double ry = ((double)cy - lay[c]) * ldx[c], dy = ldy[c], x_a = lax[c], thr = lthr[c];
#pragma unroll
        for (int i = 0; i < 4; ++i) cand |= (unsigned)(fabs(((double)cx[i] - x_a) * dy - ry) <= thr) << i;
      }
      if (!__any(cand)) continue;   // wave-uniform: no pixel of the patch is near the limb
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (!((cand >> i) & 1u)) continue;
        const bool hit = is_thick ? r_in_thick(thick[c], chw, radius, cx[i], cy, a.Ws) : r_on_line(lines[c], cx[i], cy);
        if (hit) col[i] = lcol[c];
      }
    }
    if (n == 0) continue;
    if (a.out_skel) sk_store4(a.out_skel + (size_t)f * a.skel_fs + (size_t)y * a.skel_rs + (size_t)x0 * 3, col, n);
    if (a.rgb) {
      const uint8_t* r = a.rgb + (((size_t)f * a.Ht + y) * a.Sw + (x0 + o1)) * 3;
      uint32_t rc[4] = {0u, 0u, 0u, 0u}, ov[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < n) rc[i] = (uint32_t)r[3 * i] | ((uint32_t)r[3 * i + 1] << 8) | ((uint32_t)r[3 * i + 2] << 16);
        ov[i] = col[i] == 0xFFFFFFu ? rc[i] : col[i];   // np.where(np.all(stick == 255, axis=2), rgb, stick): on the values
      }
      const size_t o = (((size_t)f * a.Ht + y) * Wo + x0) * 3;
      if (a.out_rgb) sk_store4(a.out_rgb + o, rc, n);
      if (a.out_overlay) sk_store4(a.out_overlay + o, ov, n);
    }
  }
}

extern "C" int vunet_skeleton_raster(const float* kps, int32_t F, int32_t J, const int32_t* limbs, const uint8_t* colors, int32_t L,
                                     int32_t Hs, int32_t Ws, int32_t thickness, int32_t background, const int32_t* sy,
                                     const int32_t* sx, int32_t Ht, int32_t Wt, int32_t tw, const int32_t* crop_joints,
                                     int32_t n_crop, double skel_div, double rgb_mul, const uint8_t* rgb, int32_t Sw,
                                     uint8_t* out_skel, int64_t skel_fs, int64_t skel_rs, uint8_t* out_overlay, uint8_t* out_rgb,
                                     int32_t* span, void* stream) {
  if (F < 0 || J < 1 || L < 0 || L > SK_MAXLIMB || (L > 0 && (!limbs || !colors))) return VUNET_ERR_ARG;
  if (Hs < 1 || Ws < 1 || Ht < 1 || Wt < 1 || Hs > 65535 || Ws > 65535 || Ht > 65535 || Wt > 65535) return VUNET_ERR_ARG;
  if ((!sy && Ht != Hs) || (!sx && Wt != Ws)) return VUNET_ERR_ARG;
  if (thickness < 0 || thickness > 2 * R_MAXRAD - 1 || background < 0 || background > 255) return VUNET_ERR_ARG;
  if (tw < 0 || tw > Wt || (tw > 0 && !(skel_div > 0.0)) || (crop_joints && n_crop < 1) || (span && tw == 0)) return VUNET_ERR_ARG;
  if (F == 0) return VUNET_OK;   // nothing to draw: no launch, and no pointer is looked at
  const int Wo = tw > 0 ? tw : Wt;
  if (rgb ? (tw > 0 ? Sw < tw : Sw != Wt) : (out_overlay || out_rgb)) return VUNET_ERR_ARG;
  if (!out_skel && !out_overlay && !out_rgb && !span) return VUNET_ERR_ARG;
  if (out_skel && (skel_rs < 3 * (int64_t)Wo || skel_fs < 0)) return VUNET_ERR_ARG;
  if (!kps) return VUNET_ERR_ARG;
  SkArgs a;
  a.kps = kps; a.limbs = limbs; a.colors = colors; a.sy = sy; a.sx = sx; a.crop_joints = crop_joints; a.rgb = rgb;
  a.out_skel = out_skel; a.out_overlay = out_overlay; a.out_rgb = out_rgb; a.span = span;
  a.skel_fs = skel_fs; a.skel_rs = skel_rs; a.skel_div = skel_div; a.rgb_mul = rgb_mul;
  a.J = J; a.L = L; a.Hs = Hs; a.Ws = Ws; a.thickness = thickness; a.background = background; a.Ht = Ht; a.Wt = Wt;
  a.tw = tw; a.n_crop = n_crop; a.Sw = Sw;
  const int ntiles = ((Wo + SK_TILE_W - 1) / SK_TILE_W) * ((Ht + SK_TILE_H - 1) / SK_TILE_H);
  // enough workgroups to fill the chip (256 CUs x 8 resident workgroups) when there are few frames; one workgroup, and so one
  // prologue, per frame when there are many
  int gy = 2048 / F;
  gy = gy < 1 ? 1 : (gy > ntiles ? ntiles : gy);
  if (gy > 65535) gy = 65535;
  const size_t lds = thickness > 1 ? (size_t)L * sizeof(RThick) : 0;
  VUNET_LAUNCH(skeleton_raster_kernel, dim3((unsigned)F, (unsigned)gy), dim3(256), lds, (hipStream_t)stream, a);
  return vunet_check_launch();
}
