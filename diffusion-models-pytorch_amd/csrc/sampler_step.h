// The per-element DDIM / DDPM update shared by sampler_step_kernel (elementwise.hip) and the guided steps
// (guidance.hip): reference diffusions/ddpm.py:174-252, ddim.py:57-77, CFG combine ddim.py:185 /
// ddpm.py:343-345. Written op-for-op in the reference's rounding order; both files compile with
// -ffp-contract=off, so with identical inputs the result is bit-identical to the torch CPU path.
#pragma once

#include "dm_common.h"
#include "dm_kernels.h"

namespace dm {

// predict(): model output -> (x0, eps) of element e (CFG: both branches, then the combine)
__device__ __forceinline__ void step_predict(const StepArgs& s, long e, long mo, float xt, float& x0, float& eps) {
  auto predict = [&](float out, int objective, float& px0, float& peps) {
    if (objective == 0) {
      px0 = s.c_recip * xt - s.c_recipm1 * out;
    } else if (objective == 1) {
      px0 = out;
    } else {
      px0 = s.c_sa * xt - s.c_s1ma * out;
    }
    if (s.clip) px0 = fminf(fmaxf(px0, -1.0f), 1.0f);
    peps = (s.c_recip * xt - px0) / s.c_recipm1;
  };
  if (s.out_u) {
    float x0c, epsc, x0u, epsu;
    predict(s.out_c[mo], s.objective, x0c, epsc);
    predict(s.out_u[mo], s.objective, x0u, epsu);
    const float comb = s.w_u * epsu + s.w_c * epsc;
    predict(comb, 0, x0, eps);  // hack_objective('pred_eps')
  } else {
    predict(s.out_c[mo], s.objective, x0, eps);
  }
}

// The DDIM / DDPM update of element e from its (x0, eps): writes the optional mean / x0 / eps / var
// outputs (write = false: none of them, for a caller that only needs the value again) and returns the
// sample (the caller stores it).
__device__ __forceinline__ float step_update(const StepArgs& s, long e, long mo, long per, float xt, float x0,
                                             float eps, bool write = true) {
  float mean, sample;
  if (s.kind == 0) {
    mean = s.m1 * x0 + s.m2 * eps;  // ddim.py:72-73
  } else {
    mean = s.m1 * x0 + s.m2 * xt;   // ddpm.py:230
  }
  float var = 0.f;
  float sd = s.std;
  if (s.var_mode == 1 && s.add_noise) {
    // learned_range, ddpm.py:240-246; learned channel comes from the cond branch
    const float lv = s.out_c[mo + per];
    const float frac = (lv + 1.0f) / 2.0f;
    const float logvar = frac * s.max_logvar + (1.0f - frac) * s.min_logvar;
    var = expf(logvar);
    sd = sqrtf(var);
  }
  if (s.add_noise) {
    const float nz = s.noise ? s.noise[e] : 0.f;
    sample = mean + sd * nz;
  } else {
    sample = mean;
  }
  if (write) {
    if (s.mean_out) s.mean_out[e] = mean;
    if (s.x0_out) s.x0_out[e] = x0;
    if (s.eps_out) s.eps_out[e] = eps;
    if (s.var_out) s.var_out[e] = var;
  }
  return sample;
}

// predict + update of element e (no Euler / Heun form): the unguided sample x_{t-1}
__device__ __forceinline__ float step_elem(const StepArgs& s, long e, bool write = true) {
  const long per = (long)s.C * s.HW;
  const long b = e / per, r = e - b * per;
  const long mo = b * (long)s.Cm * s.HW + r;  // model-output index of the first C channels
  const float xt = s.xt[e];
  float x0, eps;
  step_predict(s, e, mo, xt, x0, eps);
  return step_update(s, e, mo, per, xt, x0, eps, write);
}

}  // namespace dm
