// What the two forms of the behaviour path's skinny layer product, Y[B <= 64, M] = act(X[B, K] . W[M, K]^T + b), have in common
// outside their kernels (csrc/seq.hip: fp32 weights, the flow's layers and the LSTM step; csrc/seq_bf16.hip: bf16 weight
// images): the argument block, the activation, and the launchers' descriptor checks, argument fill, wave-count rule and
// dispatch over (batch tiles, waves, layout).
#pragma once
#include <type_traits>

#include "common.h"
#include "../../include/vunet_seq_tiled.h"

namespace {

constexpr int SEQ_MAX_NB = 4;   // batch tiles of 16: B <= 64

// The argument block every format shares; csrc/seq.hip extends it (behind these fields) with what the LSTM step and training add.
template <class W>
struct SeqLinearBaseArgs {
  const W* w[2];          // fp32: [M][K] row-major or tile-major images; bf16: tile images [M / 16][K / 32][64][8]
                          // (M % 16 == 0, K % 32 == 0, zero padded)
  const float* x;         // [nets_in][Bp][ldx] rows, or xt tiles [nets_in][Bp / 16][K / 32][2][64][4]
  const float* bias[2];   // [M] (NULL: none)
  float* y;               // [nets][Bp][M] rows or the next layer's xt tiles
  int M, K, Bp, ldx, act[2], shared_in;
  int S;                  // > 1: K split over grid.y workgroups, y = [nets][S][Bp][M] RAW partial slabs (no bias, no activation)
};

__device__ __forceinline__ float seq_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.01f * v);   // nn.LeakyReLU() default slope 0.01 (lib/modules.py:244)
  if (act == 2) return tanhf(v);              // the scale nets' head (lib/modules.py:252-253)
  if (act == 3) return fmaxf(v, 0.f);         // nn.ReLU: the adversarial pose regressor (models/pose_behavior_rnn.py:47-62)
  return v;
}

// ------------------------------------------------------------------------------------------------ the launchers' common part
// what every entry point asks of a descriptor (after its own pointer and layout checks)
static inline bool seq_linear_desc_ok(const vunet_seq_linear_desc* d, int layout, const void* w1) {
  if ((layout & 4) && (d->S != 1 || d->M % 32)) return false;
  if (d->nets < 1 || d->nets > 2 || (d->nets == 2 && !w1)) return false;
  if (d->B < 1 || d->B > 16 * SEQ_MAX_NB || d->M < 16 || d->M % 16) return false;
  if (d->S < 1 || d->S > 8 || d->K < 32 || d->K % (32 * d->S) || d->ldx < d->K || d->ldx % 4) return false;
  return d->act0 >= 0 && d->act0 <= 3 && d->act1 >= 0 && d->act1 <= 3;
}

template <class W>
static inline void seq_linear_fill(SeqLinearBaseArgs<W>& a, const vunet_seq_linear_desc* d, const W* w0, const W* w1, const float* x,
                                   const float* bias0, const float* bias1, float* y) {
  a.w[0] = w0;
  a.w[1] = w1;
  a.x = x;
  a.bias[0] = bias0;
  a.bias[1] = bias1;
  a.y = y;
  a.M = d->M;
  a.K = d->K;
  a.Bp = (d->B + 15) / 16 * 16;
  a.ldx = d->ldx;
  a.act[0] = d->act0;
  a.act[1] = d->act1;
  a.shared_in = d->shared_in;
  a.S = d->S;
}

// 16 waves where K gives each at least one chunk -- up to 32 batch rows.  With 3 - 4 batch tiles (the training batch of 64) a
// wave's operand loads are four times its weight loads and four waves with deeper groups are faster (flow training step at
// 64 rows: 7.77 -> 7.41 ms; at 16 rows the two forms measured the same, profiles/r05_seq_time.txt)
static inline bool seq_linear_wide(int kb, int B) { return kb >= 16 * 32 && B <= 32; }

// f(NB, WAVES, LAY) as integral constants for nb batch tiles and the layout `lay`, one of LAYS; false: nb is not 1 .. SEQ_MAX_NB
template <int V>
using seq_ic = std::integral_constant<int, V>;

template <int NB, int... LAYS, class F>
static inline void seq_dispatch_lay(bool wide, int lay, F& f) {
  ((lay == LAYS ? (wide ? f(seq_ic<NB>{}, seq_ic<16>{}, seq_ic<LAYS>{}) : f(seq_ic<NB>{}, seq_ic<4>{}, seq_ic<LAYS>{}), 0) : 0), ...);
}

template <int... LAYS, class F>
static inline bool seq_dispatch(int nb, bool wide, int lay, F f) {
  switch (nb) {
    case 1: seq_dispatch_lay<1, LAYS...>(wide, lay, f); return true;
    case 2: seq_dispatch_lay<2, LAYS...>(wide, lay, f); return true;
    case 3: seq_dispatch_lay<3, LAYS...>(wide, lay, f); return true;
    case 4: seq_dispatch_lay<4, LAYS...>(wide, lay, f); return true;
    default: return false;
  }
}

}  // namespace
