// torch.optim.Adam's update as the fused weight-gradient kernels apply it (csrc/seq_train.hip, csrc/seq_reg.hip);
// hyper-parameters: vunet_seq_adam_hp (include/vunet_seq_train.h).
#pragma once
#include "common.h"
#include "../../include/vunet_seq_train.h"

namespace {

struct AdamResolved {
  float step_size, inv_sqrt_bc2, b1, b2, eps, wd;
};

__device__ __forceinline__ AdamResolved adam_resolve(const vunet_seq_adam_hp& hp) {
  if (hp.resolved_dev) {   // formed once per step by seq_adam_tick_kernel (the same expressions): two scalar loads
    AdamResolved r;
    r.step_size = hp.resolved_dev[0];
    r.inv_sqrt_bc2 = hp.resolved_dev[1];
    r.b1 = hp.beta1;
    r.b2 = hp.beta2;
    r.eps = hp.eps;
    r.wd = hp.weight_decay;
    return r;
  }
  // bias corrections in double, as torch forms them on the host (torch/optim/adam.py: bias_correction1 / 2, step_size)
  const double t = (double)*hp.step_dev;
  const double bc1 = 1.0 - pow((double)hp.beta1, t), bc2 = 1.0 - pow((double)hp.beta2, t);
  AdamResolved r;
  r.step_size = (float)(*hp.lr_dev / bc1);
  r.inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
  r.b1 = hp.beta1;
  r.b2 = hp.beta2;
  r.eps = hp.eps;
  r.wd = hp.weight_decay;
  return r;
}

__device__ __forceinline__ void adam_update(const AdamResolved& h, float g, float& p, float& m, float& v) {
  if (h.wd != 0.f) g += h.wd * p;
  m = h.b1 * m + (1.f - h.b1) * g;
  v = h.b2 * v + (1.f - h.b2) * g * g;
  p -= h.step_size * (m / (sqrtf(v) * h.inv_sqrt_bc2 + h.eps));
}

}  // namespace
