// The routing decision of one convolution (forward / data gradient): which kernel family, which instantiation.
// conv_route() (conv_x6.hip) computes it once from the descriptor and the facts the query entry points receive; every
// launch switches on it, every *_variant formats it, publishes / wants_split are predicates on it.  Host code only.
#pragma once
#include "conv_common.h"

enum ConvFamily {
  CONV_UNSUPPORTED = 0,
  CONV_PHASE,     // (this and the next five: fp32-input kernels of vunet_conv2d_gather) strided data gradient: one generic-gather launch per output parity
  CONV_THIN,      // form = kind (1 = thin_m, 2 = thin_k), NT = 1: the column-strip form
  CONV_1X1,       // MT
  CONV_TILED,     // MT, NT, TW
  CONV_GATHER,    // MT, NT, form = KS
  CONV_SPLITK,    // form = KS
  CONV_H2_S2,     // (from here on: split kernels on a pre-split weight image, fp16 scheme) MT
  CONV_H2_SMALL,  // form = NR (0: the geometry gives no staging bound)
  CONV_H2_W16,    // MT
  CONV_H2_PAR,    // the one-launch parity form of the stride-2 data gradient
  CONV_H2,        // MT, NT
  CONV_X6,        // (bf16 scheme) MT, NT
};

struct ConvRoute {
  int family;
  int pro;          // prologue code: 0 none, 1 ELU, 2 ELU + dropout, 3 generic, 4 ReLU mask (data gradient)
  int MT, NT, TW;
  int form;         // see ConvFamily
  bool publishes;   // the launch leaves |y| maxima in GatherArgs::amax_out
};

static inline bool conv_route_is_split(const ConvRoute& r) { return r.family >= CONV_H2_S2; }

// scheme: 0 = fp32 kernels only, 1 = split-bf16 weights at hand, 2 = split-fp16 (weights and |x| maxima).  min_blocks: what
// the caller requires of the smallest row tile of a split kernel.  query: asked by an entry point that only answers.
ConvRoute conv_route(const vunet_conv_desc* d, int scheme, bool has_aux, bool has_res, bool has_mask, long min_blocks, bool query);
// the LDS-tiled fp32 kernel for prologue code `pro`, if it takes the problem (vunet_conv2d_dgrad_relu asks with pro = 4)
bool conv_route_tiled(const vunet_conv_desc* d, int pro, bool has_aux, ConvRoute* r);
// generic gather kernel for NP output pixels: CONV_SPLITK or CONV_GATHER with its <MT, NT> (the phase launches ask per parity)
int conv_route_gather_form(const vunet_conv_desc* d, long NP, int* MT, int* NT);
int conv_route_name(const ConvRoute& r, const vunet_conv_desc* d, char* name, int len);

// ---- what each family file exposes: applicability, its pick and one launch per plan (conv_route_name spells the kernels)
// conv_thin.hip: VALU kernels for the layers with <= 4 channels on one side
int vunet_conv_thin_kind(const vunet_conv_desc* d, int pro, bool has_aux, bool has_res);
bool vunet_conv_thin_strips(const vunet_conv_desc* d);
int vunet_conv_thin_launch(const ConvRoute& r, const GatherArgs& ga, hipStream_t st);
// conv_1x1.hip: streaming kernel for the 1x1 / stride-1 layers
bool vunet_conv_1x1_applicable(const vunet_conv_desc* d, int pro);
int vunet_conv_1x1_mt(const vunet_conv_desc* d);
int vunet_conv_1x1_launch(const ConvRoute& r, const GatherArgs& ga, hipStream_t st);
// conv_tiled.hip: LDS-tiled kernel for the 3x3 layers on maps at least 16 wide
bool vunet_conv_tiled_applicable(const vunet_conv_desc* d);
int vunet_conv_tiled_pick(const vunet_conv_desc* d, int* MT, bool valu_heavy);
int vunet_conv_tiled_width(const vunet_conv_desc* d);
int vunet_conv_tiled_launch(const ConvRoute& r, const GatherArgs& ga, hipStream_t st);
// conv_gather.hip: vunet_conv2d_gather with the optional |y| maxima output.  route: the caller's plan; nullptr = computed here.
int vunet_conv2d_gather_amax(const vunet_conv_desc* d, const float* x1, const float* x2, const float* wt, const float* shift,
                             const float* res, const float* aux, float* y, float* amax_out, void* stream,
                             const ConvRoute* route = nullptr);
// conv_h2_s2.hip: forward of the stride-2 layers (fp16 scheme)
bool vunet_conv_h2_s2_ok(const vunet_conv_desc* d, int pro);
int vunet_conv_h2_s2_mt(const vunet_conv_desc* d);
int vunet_conv_h2_s2_launch(const ConvRoute& r, const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, hipStream_t st);
// conv_h2_small.hip: K-split workgroups for the small maps (fp16 scheme)
bool vunet_conv_h2_small_ok(const vunet_conv_desc* d, int pro);
bool vunet_conv_h2_small_wanted(const vunet_conv_desc* d, int pro);
int vunet_conv_h2_small_nr(const vunet_conv_desc* d);
int vunet_conv_h2_small_launch(const ConvRoute& r, const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, hipStream_t st);
// conv_h2_*.hip / conv_x6_*.hip: the row-tiled split kernels, one unit per instantiation group
int vunet_conv_x6_launch_mt1(const GatherArgs& ga, const void* wx, int mtiles_pad, int pro, int NT, hipStream_t st);
int vunet_conv_x6_launch_mt2(const GatherArgs& ga, const void* wx, int mtiles_pad, int pro, int NT, hipStream_t st);
int vunet_conv_h2_launch_mt1(const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, int pro, int NT, hipStream_t st);
int vunet_conv_h2_launch_mt2(const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, int pro, int NT, hipStream_t st);
int vunet_conv_h2_launch_par(const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, hipStream_t st);
int vunet_conv_h2_launch_w16(const GatherArgs& ga, const void* wx, int mtiles_pad, const float* amax, int pro, int MT, hipStream_t st);
