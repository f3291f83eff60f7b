// optim_math.h -- the arithmetic of one parameter update, per element, for host and device (optim.hip; the host builds are
// tests/optim_host.cpp and tests/optim_modes_host.cpp): adam_onecycle (pointrcnn_amd/optim.py OneCycleAdam) first, then adam with
// L2 decay and sgd with momentum (ClipAdam, ClipSGD) below.  adam_onecycle is the reference's training recipe in its order
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

// ---- TRAIN.OPTIMIZER adam: torch.optim.Adam(lr, weight_decay=wd), the L2 decay added to the gradient (tools/train_rcnn.py:91)
//
//   g   = g_raw * coef;  g = g + wd * p             the second only with wd != 0: with wd == 0 the bits are om_update's at decay == 1
//   m, v, den as above;  p = p + neg_step * (m / den)
//
// A tensor without a gradient is not touched at all (torch skips it).  lr is the optimizer's current rate, t the parameters' step.
struct OmAdamL2 {
    float wd, omb1, beta2, omb2, bc2_sqrt, eps, neg_step;
};

OM_FN void om_adam_l2(float* p, float g_raw, float* m, float* v, float coef, const OmAdamL2& s) {
    float g = g_raw * coef;
    if (s.wd != 0.0f) {
        const float t = s.wd * *p;
        g = g + t;
    }
    const float mn = *m + s.omb1 * (g - *m);
    const float vn = *v * s.beta2 + s.omb2 * (g * g);
    const float den = sqrtf(vn) / s.bc2_sqrt + s.eps;
    *m = mn;
    *v = vn;
    *p = *p + s.neg_step * (mn / den);
}

// ---- TRAIN.OPTIMIZER sgd: torch.optim.SGD(lr, momentum, weight_decay) without dampening or Nesterov (tools/train_rcnn.py:93)
//
//   g   = g_raw * coef;  g = g + wd * p             the second only with wd != 0
//   buf = buf * momentum + g                        a zero buffer gives torch's first step (buf = g) exactly
//   p   = p + neg_lr * buf                          neg_lr = float(-lr)
//
// momentum == 0 keeps no buffer: p = p + neg_lr * g (om_sgd_plain).
struct OmSgd {
    float wd, momentum, neg_lr;
};

OM_FN float om_sgd_grad(float p, float g_raw, float coef, const OmSgd& s) {
    float g = g_raw * coef;
    if (s.wd != 0.0f) {
        const float t = s.wd * p;
        g = g + t;
    }
    return g;
}

OM_FN void om_sgd(float* p, float g_raw, float* buf, float coef, const OmSgd& s) {
    const float g = om_sgd_grad(*p, g_raw, coef, s);
    const float b = *buf * s.momentum + g;
    *buf = b;
    *p = *p + s.neg_lr * b;
}

OM_FN void om_sgd_plain(float* p, float g_raw, float coef, const OmSgd& s) {
    const float g = om_sgd_grad(*p, g_raw, coef, s);
    *p = *p + s.neg_lr * g;
}
