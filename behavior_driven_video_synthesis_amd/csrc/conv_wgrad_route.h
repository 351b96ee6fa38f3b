// The routing decision of one weight gradient: which kernel family, which instantiation, its nsplit-independent geometry and
// the slab count.  wgrad_route() (conv_wgrad.hip) computes it once from the descriptor; every launch takes it,
// wgrad_route_name() formats it, nsplit / wants_split / batchable are answers read off it.  Host code only.
#pragma once
#include "common.h"

// (the order matters to wgrad_route_wants_split)
enum WgradFamily { WGRAD_X6, WGRAD_H2, WGRAD_DIRECT, WGRAD_THIN, WGRAD_TILED, WGRAD_GENERIC };

struct WgradRoute {
  int family;
  int MTW, TH, KS, ST;              // WGRAD_X6 / WGRAD_H2: <MTW>; WGRAD_TILED: <MTW, TH, KS, ST>
  int WM, WN, NTW;                  // WGRAD_GENERIC: conv_wgrad_kernel<WM, WN, NTW>
  // WGRAD_DIRECT: geometry class (conv_wgrad_direct.hip: direct_class), kernel-row split, form = cls * 2 + rowsplit and the
  // conv_wgrad_direct_kernel<S, W4, T> it stands for; s2_ncot > 0: a launch of its own runs conv_wgrad_s2_kernel on that many
  // output-channel tiles instead (a batched launch never does: the form holds either way)
  int cls, rowsplit, form, S, W4, T, s2_ncot;
  int ncot, noct, opr, opi;         // WGRAD_DIRECT: co tiles; pixel octets in all, per output row, per image
  int ntiles, ciblocks, coblocks;   // pixel tiles (generic: 32-pixel chunks) and the grid's y, z
  int nslabs;                       // partial-result slabs the caller allocates (vunet_conv2d_wgrad_nsplit)
};

// the families whose operands are split (callers hand them tensor maxima / pre-split state): x6, h2, direct
static inline bool wgrad_route_wants_split(const WgradRoute& r) { return r.family <= WGRAD_DIRECT; }

// N * Ho * Wo up to which a direct layer is a short launch.  vunet_conv2d_wgrad_batchable reads VUNET_WGRAD_BATCH_PIX over
// it; the staged stride-2 kernel's applicability compares against the constant itself and does NOT follow the variable.
constexpr int64_t WGRAD_BATCH_PIX = 16384;

int wgrad_route_name(const WgradRoute& r, char* name, int len);

// ---- what each family file exposes: one function that fills its part of the plan (false: not its problem) and one launch
// that takes the plan.  `it` carries the descriptor with the caller's nsplit and the pointers; the grid is built at launch.
// conv_wgrad_x6.hip: 3x3 / stride 1 on the bf16 matrix cores; plans WGRAD_H2 too (d->flags bit 1): the h2 family has the x6
// applicability and slab rule, with half the workgroup target
bool vunet_wgrad_x6_plan(const vunet_wgrad_desc* d, WgradRoute* r);
int vunet_wgrad_x6_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st);
// conv_wgrad_h2.hip: the same layers with two scaled fp16 terms / three products
int vunet_wgrad_h2_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st);
// conv_wgrad_direct.hip: small maps, stride 2, 1x1 on the fp16 matrix cores (d->flags bit 1), operands straight from global
bool vunet_wgrad_direct_plan(const vunet_wgrad_desc* d, WgradRoute* r);
int vunet_wgrad_direct_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st);
// items[idx[k]] with plans routes[idx[k]], k in [0, cnt): all of one form, as few launches as hold them
int vunet_wgrad_direct_launch_multi(const vunet_wgrad_item* items, const WgradRoute* routes, const int* idx, int cnt, hipStream_t st);
// conv_wgrad_thin.hip: 3x3 layers with <= 4 output channels at full resolution (out_conv): fp32 FMA kernel
bool vunet_wgrad_thin_plan(const vunet_wgrad_desc* d, WgradRoute* r);
int vunet_wgrad_thin_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st);
// conv_wgrad_tiled.hip: LDS halo-tile fp32 kernel for 3x3 / 1x1 stride-1 and 3x3 stride-2 layers on 32-wide tiles
bool vunet_wgrad_tiled_plan(const vunet_wgrad_desc* d, WgradRoute* r);
int vunet_wgrad_tiled_launch(const WgradRoute& r, const vunet_wgrad_item& it, hipStream_t st);

// ---- the fields the kernels' argument blocks share, by name (the blocks keep their own types and layouts)
template <class Args>
static inline void wgrad_fill(Args& a, const vunet_wgrad_item& it) {
  const vunet_wgrad_desc& d = it.d;
  a.d = d;
  a.x1 = it.x1; a.x2 = it.x2; a.dy = it.dy; a.slabs = it.slabs; a.dshift = it.dshift;
  a.Ctot = d.C1 + d.C2;
  a.Coutp = (d.Cout + 31) / 32 * 32;
  a.in1 = make_inact(d.in_act, d.in_slope, d.drop_p, d.drop_seed);
  a.in2 = make_inact(d.in_act, d.in_slope, d.drop_p, d.drop_seed + 0x9E3779B9u);   // the second source's dropout stream
}

// the TH x 32 pixel tiles of x6, h2 and tiled, and how many of them a split walks
template <class Args>
static inline void wgrad_fill_tiles(Args& a, const WgradRoute& r) {
  a.tiles_per_img_w = a.d.Wo / 32;
  a.tiles_per_img = (a.d.Ho / r.TH) * a.tiles_per_img_w;
  a.ntiles = r.ntiles;
  a.tps = (r.ntiles + a.d.nsplit - 1) / a.d.nsplit;
}

// the split cap shared by the tile walkers: at most `target` workgroups, at least two tiles per split
static inline int wgrad_tile_nslabs(const WgradRoute& r, int target) {
  int S = target / (r.ciblocks * r.coblocks);
  if (S > r.ntiles / 2) S = r.ntiles / 2;
  if (S < 1) S = 1;
  return S > 512 ? 512 : S;
}
