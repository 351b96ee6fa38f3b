// Routing of the convolution path (forward / data gradient): conv_route() decides, once per call, which kernel family and
// instantiation a problem gets -- the fp32-input kernels of vunet_conv2d_gather (phase-split gather, thin, 1x1, LDS-tiled,
// gather, split-K) or the split kernels on a pre-split weight image (conv_x6_kernel.h, conv_h2_kernel.h and their stride-2 /
// small-map / 16-wide / parity forms) -- and the entry points that launch, name and answer queries from that one plan.
#include "conv_route.h"

extern "C" int vunet_x6_mtiles(int32_t M);

// VUNET_CONV_PRECISION=f32 keeps every layer on the fp32-input MFMA kernels (read once per process)
static bool x6_enabled() {
  static const bool on = [] {
    const char* e = getenv("VUNET_CONV_PRECISION");
    return !(e && (e[0] == 'f' || e[0] == 'F'));
  }();
  return on;
}

static int prologue_code(const vunet_conv_desc* d, bool has_mask) {
  if (has_mask) return (d->in_act == ACT_NONE && d->drop_p <= 0.f) ? 4 : 3;
  if (d->in_act == ACT_NONE && d->drop_p <= 0.f) return 0;
  if (d->in_act == ACT_ELU && d->drop_p <= 0.f) return 1;
  if (d->in_act == ACT_ELU) return 2;
  return 3;
}

// 16-wide staged maps (fp16 scheme only): column tiles of two rows x 16 pixels, 8-row workgroup tiles, stride 1
static bool h2_w16(const vunet_conv_desc* d) { return d->Ws % 32 != 0 && d->Ws % 16 == 0 && d->Hs % 8 == 0 && d->stride == 1; }

// geometry the kernel family covers (nothing about whether it is the fastest choice)
static bool x6_geometry_ok(const vunet_conv_desc* d, int pro, bool h2 = false) {
  if (d->KH != 3 || d->KW != 3 || d->pad != 1) return false;
  if (d->C1 <= 0 || d->C1 % 16 || d->C2 % 16 || d->Hs % 4) return false;   // Hs, Ws: the gathered (staged) map
  if (d->Ws % 32 && !(h2 && h2_w16(d))) return false;
  if (d->M % 32 || d->m_off % 32) return false;
  if (d->stride == 2)   // data gradient of the stride-2 Downsample conv: four parity launches over the dy map
    return d->mode == 1 && pro == 0 && d->C2 == 0 && d->Ho == 2 * d->Hs && d->Wo == 2 * d->Ws;
  if (d->stride != 1 || d->Hs != d->Ho || d->Ws != d->Wo) return false;
  return d->mode == 0 ? (pro == 0 || pro == 1 || pro == 2) : (pro == 0 || pro == 4);
}

static long x6_blocks(const vunet_conv_desc* d, int MT, int NT) {
  if (d->Ws % 32) return NT == 1 ? (long)d->N * (d->Hs / 8) * (d->Ws / 16) * ((d->M + 32 * MT - 1) / (32 * MT)) : 0;  // h2_w16
  if (d->Hs % (4 * NT)) return 0;
  return (long)d->N * (d->Hs / (4 * NT)) * (d->Ws / 32) * ((d->M + 32 * MT - 1) / (32 * MT));
}

// Tile: M <= 32 -> one m-tile and up to 16 rows (the weight slab is re-staged per workgroup: tall tiles amortise it);
// wider layers -> two m-tiles and 8 rows (LDS: two workgroups per CU).  The tallest tile that still gives every CU its
// two resident workgroups wins; `min_blocks` is what the caller requires of the smallest tile.
static int x6_pick(const vunet_conv_desc* d, int* MT, long min_blocks, bool h2 = false) {
  *MT = d->M <= 32 ? 1 : 2;
  // bf16 scheme: up to 16 rows for one m-tile.  fp16 scheme (two accumulator sets): 8 rows for two m-tiles; one m-tile
  // runs best on 4-row tiles -- 113 VGPRs and 38 KB of LDS let FOUR workgroups share a CU, which hides more of the short-K
  // layers' load / store phases (32 channels at 256^2: 120 -> 112 us, r02)
  const int top = h2 ? (*MT == 1 ? 1 : 2) : (*MT == 1 ? 4 : 2);
  if (int NT = g_vunet_tune[VUNET_TUNE_SPLIT_FORCE_NT]) {  // tests / tuning (vunet_set_tuning)
    if (NT > top) NT = (h2 && *MT == 1 && NT == 2) ? 2 : top;   // (h2, one m-tile: the 8-row form is built, for A/B runs)
    if ((NT == 1 || NT == 2 || NT == 4) && x6_blocks(d, *MT, NT) > 0) return NT;
  }
  // (r03: one m-tile per workgroup for the 16-wide maps -- VGG19 conv5_x at bs 16 is 256 workgroups of two m-tiles, half of
  //  the residency slots empty -- measured no faster forward (92 us either way) and 6 % slower data gradient: a chunk's time
  //  there is its staging, the same for one m-tile as for two)
  for (int NT = top; NT >= 2; NT >>= 1)
    if (x6_blocks(d, *MT, NT) >= 512) return NT;
  // (r03: one m-tile per workgroup for the 128-channel 32^2 layers -- 512 workgroups instead of 256 -- measured no
  //  different: 27.7 / 26.2 us either way; these launches are latency-bound, not short of parallelism)
  return x6_blocks(d, *MT, 1) >= min_blocks ? 1 : 0;
}

// ---- the fp32-input half: vunet_conv2d_gather's kernels
VUNET_ENV_FLAG(env_no_tiled, "VUNET_NO_TILED")
VUNET_ENV_FLAG(env_no_phase, "VUNET_NO_PHASE")

// Few output tiles and a long K: share each tile's K loop between 16 waves.  Up to 768 tiles (3 per CU) any layer
// with >= 64 input channels; up to 2048 tiles only when K is at least 576 deep (3x3 over >= 64 channels) -- there
// the one-wave-per-tile kernel is latency bound (25 x 256->128 @ 16^2: 582 us vs ~60 us split).
static bool want_splitk(const vunet_conv_desc* d, long NP, int taps) {
  const long tiles = ((NP + 31) / 32) * ((d->M + 31) / 32);
  const int kpairs = ((d->C1 + 1) >> 1) + ((d->C2 + 1) >> 1);
  return (tiles <= 768 && kpairs >= 32) || (tiles <= 2048 && (long)kpairs * taps >= 288);
}

int conv_route_gather_form(const vunet_conv_desc* d, long NP, int* MT, int* NT) {
  *MT = *NT = 1;
  if (want_splitk(d, NP, d->KH * d->KW)) return CONV_SPLITK;
  if (d->M <= 32) *NT = 4;
  else *MT = *NT = 2;
  return CONV_GATHER;
}

bool conv_route_tiled(const vunet_conv_desc* d, int pro, bool has_aux, ConvRoute* r) {
  if (env_no_tiled() || !vunet_conv_tiled_applicable(d) ||
      !(d->mode == 0 ? pro != 4 : (pro == 0 || (pro == 4 && d->stride == 1))) || pro == 3)
    return false;
  // quirk, kept: whether the family takes the problem is asked with valu_heavy = true, the tile it then runs with the real value
  if (vunet_conv_tiled_pick(d, &r->MT, true) <= 0) return false;
  r->family = CONV_TILED, r->pro = pro, r->form = 0;
  r->NT = vunet_conv_tiled_pick(d, &r->MT, (pro != 0 && pro != 4) || (d->mode == 1 && has_aux));
  r->TW = vunet_conv_tiled_width(d);
  r->publishes = !d->d2s;
  return true;
}

static ConvRoute gather_route(const vunet_conv_desc* d, bool has_aux, bool has_res) {
  ConvRoute r = {CONV_UNSUPPORTED, prologue_code(d, false), 1, 1, 32, 0, false};
  const long NP = (long)d->N * d->Ho * d->Wo;
  if (d->mode == 1 && d->stride > 1 && !env_no_phase()) {
    r.family = CONV_PHASE;
  } else if (const int thin = vunet_conv_thin_kind(d, r.pro, has_aux, has_res)) {
    r.family = CONV_THIN, r.form = thin;
    r.NT = vunet_conv_thin_strips(d) ? 1 : 0;
    r.publishes = thin == 2;   // the 3-channel-input kernel publishes (no thin kernel stores depth-to-space)
  } else if (vunet_conv_1x1_applicable(d, r.pro) && !want_splitk(d, NP, 1)) {
    // the streaming 1x1 kernel, unless the problem is so small that splitting K over 16 waves is the better plan
    r.family = CONV_1X1, r.MT = vunet_conv_1x1_mt(d);
    r.publishes = !d->d2s;
  } else if (!conv_route_tiled(d, r.pro, has_aux, &r)) {
    r.family = conv_route_gather_form(d, NP, &r.MT, &r.NT);
    r.form = (d->KH == 3 && d->KW == 3) ? 3 : ((d->KH == 1 && d->KW == 1) ? 1 : 0);
    r.publishes = r.family == CONV_SPLITK && !d->d2s;   // (the one-wave-per-tile kernel does not publish)
  }
  return r;
}

// ---- the split half.  CONV_UNSUPPORTED: no split kernel takes the problem.
static ConvRoute split_route(const vunet_conv_desc* d, bool h2, bool has_aux, bool has_res, bool has_mask, long min_blocks,
                             bool query) {
  ConvRoute r = {CONV_UNSUPPORTED, prologue_code(d, has_mask), 0, 0, 32, 0, h2};   // only the fp16 kernels publish |y| maxima
  const int pro = r.pro;
  if (h2 && !has_mask && !has_aux && !has_res && !g_vunet_tune[VUNET_TUNE_S2_FWD_F32] && vunet_conv_h2_s2_ok(d, pro)) {
    r.family = CONV_H2_S2, r.MT = vunet_conv_h2_s2_mt(d);   // stride-2 forward: its own kernel (parity-plane staging)
    return r;
  }
  r.NT = x6_geometry_ok(d, pro, h2) ? x6_pick(d, &r.MT, min_blocks, h2) : 0;
  // quirk, kept: VUNET_TUNE_FORCE_SMALL (tests) moves the launch only; the queries and the names do not see it
  if (!query && g_vunet_tune[VUNET_TUNE_FORCE_SMALL] && h2 && !has_mask && vunet_conv_h2_small_ok(d, pro)) r.NT = 0;
  if (r.NT == 0) {
    // the row-tiled kernels do not cover / cannot fill the chip with this problem: the small-map form (fp16 scheme), which
    // publishes through every store, depth-to-space included
    if (!h2 || has_mask || !(min_blocks <= 1 ? vunet_conv_h2_small_ok(d, pro) : vunet_conv_h2_small_wanted(d, pro))) return r;
    r.family = CONV_H2_SMALL, r.form = vunet_conv_h2_small_nr(d);
  } else if (!h2) {
    r.family = CONV_X6;
  } else if (d->Ws % 32) {
    r.family = CONV_H2_W16, r.TW = 16;
  } else if (d->stride == 2 && !g_vunet_tune[VUNET_TUNE_PARITY_LAUNCHES]) {
    r.family = CONV_H2_PAR;   // (stride 2 passed x6_geometry_ok: a data gradient) all four output parities in one launch
  } else {
    r.family = CONV_H2;       // two-term fp16 image
  }
  return r;
}

// would vunet_conv2d route this problem to a split kernel?  Big enough to fill the chip, not a 3-channel layer.
ConvRoute conv_route(const vunet_conv_desc* d, int scheme, bool has_aux, bool has_res, bool has_mask, long min_blocks, bool query) {
  if (scheme != 0 && x6_enabled()) {
    const int pro = prologue_code(d, has_mask);
    if (vunet_conv_thin_kind(d, pro == 4 ? 0 : pro, has_aux, has_res) == 0) {
      const ConvRoute r = split_route(d, scheme == 2, has_aux, has_res, has_mask, min_blocks, query);
      if (r.family != CONV_UNSUPPORTED) return r;
      // quirk, kept: a launch that FORCE_SMALL took off a row-tiled kernel and the small-map form then refuses (more than 2048
      // tiles) is refused -- CONV_UNSUPPORTED -- not rerouted to the fp32 kernels
      if (!query && g_vunet_tune[VUNET_TUNE_FORCE_SMALL] &&
          split_route(d, scheme == 2, has_aux, has_res, has_mask, min_blocks, true).family != CONV_UNSUPPORTED)
        return r;
    }
  }
  return gather_route(d, has_aux, has_res);
}

// the kernel's name in rocprofv3's spelling (bench.py and the timing tools match it against the kernel trace)
int conv_route_name(const ConvRoute& r, const vunet_conv_desc* d, char* name, int len) {
  switch (r.family) {
    case CONV_PHASE: snprintf(name, len, "conv_gather_kernel<phase x%d>", d->stride * d->stride); break;
    case CONV_THIN:
      if (r.form == 1 && r.NT == 1) snprintf(name, len, "conv_thin_mv_kernel<%d, 4>", d->mode);
      else if (r.form == 1) snprintf(name, len, "conv_thin_m_kernel<%d>", d->mode);
      else if (r.NT == 1) snprintf(name, len, "conv_thin_kv_kernel<3, 4>");
      else snprintf(name, len, "conv_thin_k_kernel<%d, 3>", d->KH);
      break;
    case CONV_1X1: snprintf(name, len, "conv_1x1_kernel<%d, %d, %d>", r.MT, d->mode, d->mode == 1 ? 0 : r.pro); break;
    case CONV_TILED: {
      const int nt = r.TW == 16 ? 1 : r.NT;
      snprintf(name, len, "conv_tiled_kernel<%d, %d, %d, %d, %d, %d, %d>", r.MT, d->stride == 2 ? 1 : nt,
               (r.MT == 2 && nt == 4) ? 4 : 8, d->mode, d->mode == 1 ? (r.pro == 4 ? 4 : 0) : r.pro, r.TW, d->stride);
      break;
    }
    case CONV_GATHER: snprintf(name, len, "conv_gather_kernel<%d, %d, %d, %d>", r.MT, r.NT, r.pro, r.form); break;
    case CONV_SPLITK: snprintf(name, len, "conv_gather_splitk_kernel<16, %d, %d>", r.pro, r.form); break;
    case CONV_H2_S2: snprintf(name, len, "conv_h2_s2_kernel<%d>", r.MT); break;
    case CONV_H2_SMALL:
      if (r.form == 0) return VUNET_ERR_UNSUPPORTED;
      snprintf(name, len, "conv_h2_small_kernel<%d, %d>", r.pro, r.form); break;
    case CONV_H2_W16: snprintf(name, len, "conv_h2_kernel<%d, 1, %d, %d, -1, 4, 16>", r.MT, d->mode, r.pro); break;
    case CONV_H2_PAR: snprintf(name, len, "conv_h2_kernel<1, 1, 1, 0, 4, 4, 32>"); break;
    case CONV_H2:
      if (d->stride == 2) snprintf(name, len, "conv_h2_kernel<%d, %d, 1, 0, parity x4, 4, 32>", r.MT, r.NT);
      else snprintf(name, len, "conv_h2_kernel<%d, %d, %d, %d, -1, 4, 32>", r.MT, r.NT, d->mode, r.pro);
      break;
    case CONV_X6:
      if (d->stride == 2) snprintf(name, len, "conv_x6_kernel<%d, %d, 1, 0, parity x4>", r.MT, r.NT);
      else snprintf(name, len, "conv_x6_kernel<%d, %d, %d, %d, -1>", r.MT, r.NT, d->mode, r.pro);
      break;
    default: return VUNET_ERR_UNSUPPORTED;
  }
  return VUNET_OK;
}

// ---- launches
static int split_launch(const ConvRoute& r, const vunet_conv_desc* d, const float* x1, const float* x2, const void* wx,
                        const float* shift, const float* res, const float* aux, const float* mask, float* y, const float* amax,
                        float* amax_out, void* stream, const float* amax2 = nullptr, const float* res2 = nullptr) {
  if (res2 && (d->mode != 1 || !amax)) return VUNET_ERR_UNSUPPORTED;   // (second residual: the fp16 scheme's data gradients)
  if (r.family == CONV_UNSUPPORTED) return VUNET_ERR_UNSUPPORTED;
  GatherArgs ga;
  fill_gather_args(ga, d, x1, x2, nullptr, shift, res, aux, mask, y, d->stride == 1 && d->Wo % 4 == 0);
  ga.amax2 = amax2;
  if (r.publishes) ga.amax_out = amax_out;
  hipStream_t st = (hipStream_t)stream;
  // K dimension of the image = the gathered tensor's channels; M dimension = all columns of the weight matrix
  const int mtp = vunet_x6_mtiles(d->Mpad);
  if (r.family == CONV_H2_S2) return vunet_conv_h2_s2_launch(r, ga, wx, mtp, amax, st);   // (no residuals on this route)
  ga.res2 = res2;
  // the 16-byte epilogue reads res2 with float4 loads too: an offset view that is contiguous but not 16-byte aligned
  // takes the scalar epilogue
  ga.wide = ga.wide && (reinterpret_cast<uintptr_t>(res2) & 15) == 0;
  switch (r.family) {
    case CONV_H2_SMALL: return vunet_conv_h2_small_launch(r, ga, wx, mtp, amax, st);
    case CONV_H2_W16: return vunet_conv_h2_launch_w16(ga, wx, mtp, amax, r.pro, r.MT, st);
    case CONV_H2_PAR: return vunet_conv_h2_launch_par(ga, wx, mtp, amax, st);
    case CONV_H2:
      return r.MT == 1 ? vunet_conv_h2_launch_mt1(ga, wx, mtp, amax, r.pro, r.NT, st)
                       : vunet_conv_h2_launch_mt2(ga, wx, mtp, amax, r.pro, r.NT, st);
    default:
      return r.MT == 1 ? vunet_conv_x6_launch_mt1(ga, wx, mtp, r.pro, r.NT, st)
                       : vunet_conv_x6_launch_mt2(ga, wx, mtp, r.pro, r.NT, st);
  }
}

extern "C" int vunet_conv2d_x6(const vunet_conv_desc* d, const float* x1, const float* x2, const void* wx,
                               const float* shift, const float* res, const float* aux, const float* mask, float* y,
                               const float* amax, float* amax_out, void* stream) {
  if (!d || !x1 || !wx || !y || (d->C2 > 0 && !x2) || d->Mpad % 32 != 0) return VUNET_ERR_ARG;
  if (mask && (d->mode != 1 || d->C2 != 0)) return VUNET_ERR_ARG;
  if (d->d2s && (d->M % 4 != 0 || d->mode != 0)) return VUNET_ERR_ARG;
  // the split kernels or nothing: no look at VUNET_CONV_PRECISION or the thin layers, and any tile that covers the problem
  const ConvRoute r = split_route(d, amax != nullptr, aux != nullptr, res != nullptr, mask != nullptr, 1, false);
  return split_launch(r, d, x1, x2, wx, shift, res, aux, mask, y, amax, amax_out, stream);
}

extern "C" int vunet_conv2d_a2(const vunet_conv_desc* d, const float* x1, const float* x2, const float* wt, const void* wx,
                               const float* shift, const float* res, const float* res2, const float* aux, float* y,
                               const float* amax, const float* amax2, float* amax_out, void* stream) {
  if (!d) return VUNET_ERR_ARG;
  if (amax2 && (!amax || d->C2 <= 0)) return VUNET_ERR_ARG;
  if (res2 && (!res || d->mode != 1)) return VUNET_ERR_ARG;
  if (!wx) {   // fp32 kernels only: vunet_conv2d_gather checks its arguments before it routes
    if (res2) return VUNET_ERR_UNSUPPORTED;
    return vunet_conv2d_gather_amax(d, x1, x2, wt, shift, res, aux, y, amax_out, stream);
  }
  const ConvRoute r = conv_route(d, amax ? 2 : 1, aux != nullptr, res != nullptr, false, 128, false);
  if (conv_route_is_split(r) || r.family == CONV_UNSUPPORTED) {   // (unsupported: split_launch answers so)
    if (!x1 || !y || (d->C2 > 0 && !x2) || d->Mpad % 32 != 0) return VUNET_ERR_ARG;
    return split_launch(r, d, x1, x2, wx, shift, res, aux, nullptr, y, amax, amax_out, stream, amax2, res2);
  }
  if (res2) return VUNET_ERR_UNSUPPORTED;   // (the fp32 kernels take one residual: the caller adds the second itself)
  return vunet_conv2d_gather_amax(d, x1, x2, wt, shift, res, aux, y, amax_out, stream, &r);
}

extern "C" int vunet_conv2d(const vunet_conv_desc* d, const float* x1, const float* x2, const float* wt, const void* wx,
                            const float* shift, const float* res, const float* aux, float* y, const float* amax,
                            float* amax_out, void* stream) {
  return vunet_conv2d_a2(d, x1, x2, wt, wx, shift, res, nullptr, aux, y, amax, nullptr, amax_out, stream);
}

extern "C" int vunet_conv2d_dgrad_relu_x6(const vunet_conv_desc* d, const float* dy, const float* y, const void* wx,
                                          const float* res, float* dx, const float* amax, float* amax_out, void* stream) {
  if (!d || !dy || !y || !wx || !dx || d->mode != 1 || d->C2 != 0 || d->Mpad % 32 != 0) return VUNET_ERR_ARG;
  if (d->aux_act != ACT_NONE || d->aux_drop_p > 0.f) return VUNET_ERR_UNSUPPORTED;
  const ConvRoute r = conv_route(d, amax ? 2 : 1, false, res != nullptr, true, 128, false);
  if (!conv_route_is_split(r)) return VUNET_ERR_UNSUPPORTED;
  return split_launch(r, d, dy, nullptr, wx, nullptr, res, nullptr, y, dx, amax, amax_out, stream);
}

// ---- queries: predicates on the plan, and its name
extern "C" int vunet_conv2d_x6_supported(const vunet_conv_desc* d, int32_t has_mask) {
  return d && x6_geometry_ok(d, prologue_code(d, has_mask != 0)) ? 1 : 0;
}

extern "C" int vunet_conv2d_wants_split(const vunet_conv_desc* d, int32_t has_aux, int32_t has_res, int32_t has_mask, int32_t split) {
  // quirk, kept: split = 0 is answered as the bf16 scheme
  return d && conv_route_is_split(conv_route(d, split == 2 ? 2 : 1, has_aux != 0, has_res != 0, has_mask != 0, 128, true)) ? 1 : 0;
}

extern "C" int vunet_conv2d_publishes_amax(const vunet_conv_desc* d, int32_t has_aux, int32_t has_res, int32_t split) {
  if (!d) return 0;
  return conv_route(d, split == 0 ? 0 : (split == 2 ? 2 : 1), has_aux != 0, has_res != 0, false, 128, true).publishes ? 1 : 0;
}

// Name (rocprofv3 spelling) of the kernel vunet_conv2d_gather would launch for this problem.
extern "C" int vunet_conv2d_gather_variant(const vunet_conv_desc* d, int32_t has_aux, char* name, int32_t len) {
  if (!d || !name || len < 8) return VUNET_ERR_ARG;
  // quirk, kept: this entry point has no has_res, and a residual keeps a layer off the 3-channel-input thin kernel
  return conv_route_name(gather_route(d, has_aux != 0, false), d, name, len);
}

// Name (rocprofv3 spelling) of the kernel vunet_conv2d / vunet_conv2d_dgrad_relu_x6 launches for this problem.
extern "C" int vunet_conv2d_variant(const vunet_conv_desc* d, int32_t has_aux, int32_t has_wx, int32_t has_mask,
                                    char* name, int32_t len) {
  if (!d || !name || len < 8) return VUNET_ERR_ARG;
  // quirk, kept: asked with has_res = false, whatever the launch will be given (see vunet_conv2d_gather_variant)
  return conv_route_name(conv_route(d, has_wx == 2 ? 2 : (has_wx ? 1 : 0), has_aux != 0, false, has_mask != 0, 128, true), d,
                         name, len);
}
