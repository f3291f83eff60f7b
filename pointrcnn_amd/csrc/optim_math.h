// optim_math.h -- the arithmetic of one adam_onecycle parameter update (pointrcnn_amd/optim.py OneCycleAdam), per element, for
// host and device (optim.hip; the host build is tests/optim_host.cpp).  It is the reference's training recipe in its order
// (tools/train_utils/train_utils.py:135 clip_grad_norm_, fastai_optim.py:132-149 OptimWrapper.step's decoupled decay, then
// torch.optim.Adam.step), every operation individually rounded in float32 (the library is built with -ffp-contract=off; division
// and square root are correctly rounded, -fhip-fp32-correctly-rounded-divide-sqrt):
//
//   g   = g_raw * coef                              coef = min(max_norm / (norm + 1e-6), 1) in float32; always applied, as torch does
//   p   = p * decay                                 decay    = float(1 - wd * lr)
//   m   = m + omb1 * (g - m)                        omb1     = float(1 - beta1)
//   v   = v * beta2 + omb2 * (g * g)                beta2, omb2 = float(beta2), float(1 - beta2)
//   den = sqrt(v) / bc2_sqrt + eps                  bc2_sqrt = float(sqrt(1 - beta2^t))
//   p   = p + neg_step * (m / den)                  neg_step = float(-(lr / (1 - beta1^t)))
//
// The scalars are formed on the host in double, the way torch forms them from Python floats, and rounded to float32 ONCE
// (optim.py adam_scalars); nothing here calls pow.  lr and beta1 are the schedule's values of iteration t - 1, t counted from 1.
// A tensor without a gradient receives the decay alone (om_decay): its moments are not touched.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define OM_FN __host__ __device__ __forceinline__

struct OmScalars {
    float decay, omb1, beta2, omb2, bc2_sqrt, eps, neg_step;
};

// norm: the float32 rounding of the global 2-norm of all gradients.  A NaN norm gives a NaN coefficient (torch.clamp keeps it).
OM_FN float om_clip_coef(float norm, float max_norm) {
    const float c = max_norm / (norm + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}

OM_FN float om_decay(float p, const OmScalars& s) { return p * s.decay; }

OM_FN void om_update(float* p, float g_raw, float* m, float* v, float coef, const OmScalars& s) {
    const float g = g_raw * coef;
    const float pd = *p * s.decay;
    const float mn = *m + s.omb1 * (g - *m);
    const float vn = *v * s.beta2 + s.omb2 * (g * g);
    const float den = sqrtf(vn) / s.bc2_sqrt + s.eps;
    *m = mn;
    *v = vn;
    *p = pd + s.neg_step * (mn / den);
}
