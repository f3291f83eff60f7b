// rpn_loss_math.h -- the arithmetic of the RPN training loss (pointrcnn_amd/train_functions.py get_rpn_loss + get_reg_loss, i.e.
// lib/net/train_functions.py:54-127 and lib/utils/loss_utils.py:25-253) for one row, for host and device (rpn_loss.hip; the host
// build is tests/rpn_loss_math_host.cpp).
//
// Label targets -- the contract is torch's CPU float32 sequence, bit for bit (it is what generated tests/golden/train_ref.npz):
//   * a Python double constant (scope, 2*scope - 1e-3, bin_size, bin_size/2, 2*pi, apc, apc/2, the anchor) is rounded to float32
//     ONCE, on the host (rl_make_config), before use;
//   * every operation is individually rounded (the library is built with -ffp-contract=off) and division is true IEEE division
//     (-fhip-fp32-correctly-rounded-divide-sqrt);
//   * `%` is torch.remainder: fmodf, then + divisor when the result is non-zero and its sign differs from the divisor's.
//   _bin_and_residual:  shift = clamp(off + scope, 0, 2*scope - 1e-3); bin = floor(shift / bin_size);
//                       res = (shift - (float(bin) * bin_size + bin_size/2)) / bin_size
//   angle (get_ry_fine=False): shift = ((ry % 2pi) + apc/2) % 2pi; bin = clamp(floor(shift / apc), 0, num_head_bin - 1);
//                       res = (shift - (float(bin) * apc + apc/2)) / (apc/2)
//   size:               (hwl - anchor) / anchor
// torch on the GPU may divide by a host scalar as a multiply by its reciprocal.  For bin_size = 0.5 that is exact; for
// apc = pi/6 it is not, so torch-CPU and torch-GPU can put a label that sits within an ulp of an angle-bin edge into different
// bins.  The CPU sequence is the contract here.
// Bins are clamped into their range whatever the label (a NaN label gives bin 0): they index memory.
//
// Per-row terms and derivatives (float32, the composed code's own expressions; compared with float64 closed forms, not bitwise):
//   focal:      ce = max(x,0) - x*t + log1p(exp(-|x|)); p = sigmoid(x); p_t = t*p + (1-t)*(1-p); mod = (1-p_t)^gamma;
//               a = t*alpha + (1-t)*(1-alpha); term = mod * a * ce * w          d/dx = a * w * (dmod*ce + mod*(p - t))
//   softmax CE: log(sum exp(z - max)) - (z[target] - max)                       d/dz_j = exp((z_j - max) - logsum) - [j == target]
//   smooth-L1:  d = a - b; |d| < 1 ? 0.5*d*d : |d| - 0.5                        d/da = |d| < 1 ? d : sign(d)
//
// The other two RPN.LOSS_CLS kinds (train_functions.get_rpn_loss, lib/net/train_functions.py:66-90, lib/utils/loss_utils.py:7-21),
// p = sigmoid(x) = 1 / (1 + exp(-x)) in float32, t = [label > 0]:
//   BCE:   F.binary_cross_entropy(p, t, weight=w) with w = FG_WEIGHT (rounded to float32 once) for a foreground row, 1 otherwise:
//               term = ((t-1) * max(log1p(-p), -100) - t * max(log(p), -100)) * w
//               d/dx = ((p - t) / max((1-p)*p, 1e-12)) * w * (1-p) * p     (autograd: the BCE backward, then sigmoid's)
//          the caller sums the terms of the valid rows and scales the sum by norm[0] (1 / max(valid, 1), or world / global valid)
//   Dice:  lo = min(p, t), hi = max(p, t); with A = sum lo, B = sum hi over the valid rows (the caller's, in double) the loss is
//          1 - A / max(B, 1) and d/dx = s * (-dlo / max(B, 1) + [B >= 1] * A / max(B, 1)^2 * dhi), where
//               dlo = (1-p)*p for t = 1, else 0;      dhi = (1-p)*p for t = 0, else 0
// Where float32 sigmoid saturates: from x ~ 17 on, 1 + exp(-x) rounds to 1 and p == 1; p == 0 only once exp(-x) overflows
// (x < -88.7), but 1 - p == 1 already from x ~ -17 down.  With p == 1: (1-p)*p == 0, so both derivatives are exactly 0; the BCE
// term is 100 w against t = 0 (log1p(-1) = -inf, clamped) and 0 against t = 1; Dice has lo = t, hi = 1.  With p == 0: the
// derivatives are exactly 0 again (the BCE quotient is finite through its 1e-12 floor), the BCE term is 100 w against t = 1 and 0
// against t = 0; Dice has lo = 0, hi = t.  In between (-88 < x < -17) the BCE term against t = 1 is -log(p) ~ -x, exact to float32,
// and against t = 0 it is -log1p(-p) ~ p.  This is the composed float32 code's behaviour, value for value; float64 keeps
// a non-zero derivative up to |x| ~ 37.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define RL_FN __host__ __device__ __forceinline__

constexpr int RL_MAX_BINS = 16;           // nb and num_head_bin the kernels accept; ops.RPN_LOSS_MAX_BINS
constexpr int RL_TERMS = 11;              // cls cls_pos cls_neg x_bin z_bin x_res z_res y_offset ry_bin ry_res size
enum { RL_CLS = 0, RL_CLS_POS, RL_CLS_NEG, RL_X_BIN, RL_Z_BIN, RL_X_RES, RL_Z_RES, RL_Y_OFF, RL_RY_BIN, RL_RY_RES, RL_SIZE };
constexpr int RL_KIND_FOCAL = 0, RL_KIND_DICE = 1, RL_KIND_BCE = 2;      // RPN.LOSS_CLS, ops.rpn_loss_cfg's numbering

struct RlConfig {
    float scope, shift_hi, bin, half_bin;     // LOC_SCOPE, 2*LOC_SCOPE - 1e-3, LOC_BIN_SIZE, LOC_BIN_SIZE/2
    float two_pi, apc, half_apc;              // 2*pi, 2*pi/num_head_bin, pi/num_head_bin
    float anchor[3];                          // MEAN_SIZE
    float alpha, gamma;                       // focal loss; has_alpha 0: no alpha weighting
    int has_alpha;
    int nb, nh, xz_fine, C;                   // bins per x/z head, angle bins, LOC_XZ_FINE, channels of a regression row
    double w_cls, w_reg;                      // LOSS_WEIGHT
};

// constants as Python forms them in double, rounded to float32 once
static inline RlConfig rl_make_config(double loc_scope, double loc_bin_size, int num_head_bin, int xz_fine, const double* mean_size,
                                      double gamma, double alpha, int has_alpha, double w_cls, double w_reg) {
    RlConfig c;
    const double two_pi = 2.0 * 3.141592653589793;
    const double apc = two_pi / num_head_bin;
    c.scope = (float)loc_scope;
    c.shift_hi = (float)(loc_scope * 2 - 1e-3);
    c.bin = (float)loc_bin_size;
    c.half_bin = (float)(loc_bin_size / 2);
    c.two_pi = (float)two_pi;
    c.apc = (float)apc;
    c.half_apc = (float)(apc / 2);
    for (int k = 0; k < 3; ++k) c.anchor[k] = (float)mean_size[k];
    c.alpha = (float)alpha;
    c.gamma = (float)gamma;
    c.has_alpha = has_alpha;
    c.nb = (int)(loc_scope / loc_bin_size) * 2;
    c.nh = num_head_bin;
    c.xz_fine = xz_fine;
    c.C = (xz_fine ? 4 : 2) * c.nb + 1 + 2 * c.nh + 3;
    c.w_cls = w_cls;
    c.w_reg = w_reg;
    return c;
}

// ---------------------------------------------------------------------------------------------- label targets (bitwise contract)
RL_FN float rl_remainder(float a, float b) {
    float m = fmodf(a, b);
    if (m != 0.0f && ((b < 0.0f) != (m < 0.0f))) m = m + b;
    return m;
}

// floor'ed quotient -> a bin in [0, n-1]
RL_FN int rl_bin_index(float f, int n) {
    const float hi = (float)(n - 1);
    return f >= hi ? n - 1 : (f > 0.0f ? (int)f : 0);
}

RL_FN void rl_bin_and_residual(float off, const RlConfig& c, int* bin, float* res) {
    float s = off + c.scope;
    s = s < 0.0f ? 0.0f : s;
    s = s > c.shift_hi ? c.shift_hi : s;
    const int b = rl_bin_index(floorf(s / c.bin), c.nb);
    *bin = b;
    *res = (s - ((float)b * c.bin + c.half_bin)) / c.bin;
}

RL_FN void rl_angle_bin_and_residual(float ry, const RlConfig& c, int* bin, float* res) {
    const float s = rl_remainder(rl_remainder(ry, c.two_pi) + c.half_apc, c.two_pi);
    const int b = rl_bin_index(floorf(s / c.apc), c.nh);
    *bin = b;
    *res = (s - ((float)b * c.apc + c.half_apc)) / c.half_apc;
}

RL_FN float rl_size_target(float v, float anchor) { return (v - anchor) / anchor; }

// ---------------------------------------------------------------------------------------------- per-row terms
// focal term of one point with target t in {0, 1} and weight w, and its derivative in the logit
RL_FN void rl_focal(float x, float t, float w, const RlConfig& c, float* val, float* dx) {
    float ce = fmaxf(x, 0.0f) - x * t;
    ce = ce + log1pf(expf(-fabsf(x)));
    const float p = 1.0f / (1.0f + expf(-x));
    const float p_t = t * p + (1.0f - t) * (1.0f - p);
    const float q = 1.0f - p_t;
    const float dq = (1.0f - 2.0f * t) * (p * (1.0f - p));
    float mod = 1.0f, dmod = 0.0f;
    if (c.gamma == 2.0f) {
        mod = q * q;
        dmod = 2.0f * q * dq;
    } else if (c.gamma != 0.0f) {
        mod = powf(q, c.gamma);
        dmod = q > 0.0f ? c.gamma * powf(q, c.gamma - 1.0f) * dq : 0.0f;
    }
    const float a = c.has_alpha ? t * c.alpha + (1.0f - t) * (1.0f - c.alpha) : 1.0f;
    *val = mod * a * ce * w;
    *dx = a * w * (dmod * ce + mod * (p - t));
}

// BinaryCrossEntropy term of one point with target t in {0, 1} and weight w, and its derivative in the logit (the operation order
// of F.binary_cross_entropy and of its and sigmoid's backward; the header comment says what saturation gives)
RL_FN void rl_bce(float x, float t, float w, float* val, float* dx) {
    const float p = 1.0f / (1.0f + expf(-x));
    const float q = 1.0f - p;
    const float v = (t - 1.0f) * fmaxf(log1pf(-p), -100.0f) - t * fmaxf(logf(p), -100.0f);
    *val = v * w;
    float d = (p - t) / fmaxf(q * p, 1e-12f);
    d = d * w;
    d = d * q;
    *dx = d * p;
}

// DiceLoss addends of one point with target t in {0, 1}: min(p, t), max(p, t) and their derivatives in the logit (one of them is 0)
RL_FN void rl_dice(float x, float t, float* lo, float* hi, float* dlo, float* dhi) {
    const float p = 1.0f / (1.0f + expf(-x));
    const float dp = (1.0f - p) * p;
    *lo = fminf(p, t);
    *hi = fmaxf(p, t);
    *dlo = t > 0.0f ? dp : 0.0f;
    *dhi = t > 0.0f ? 0.0f : dp;
}

// the same for a row by its label (rl_label's -1 ignored, 0 background, 1 foreground): an ignored row contributes zeros; a
// foreground row of the BCE sum weighs fg_weight, a background row 1
RL_FN void rl_bce_row(float x, int label, float fg_weight, float* val, float* dx) {
    *val = 0.0f;
    *dx = 0.0f;
    if (label >= 0) rl_bce(x, (float)label, label > 0 ? fg_weight : 1.0f, val, dx);
}

RL_FN void rl_dice_row(float x, int label, float* lo, float* hi, float* dlo, float* dhi) {
    *lo = *hi = *dlo = *dhi = 0.0f;
    if (label >= 0) rl_dice(x, (float)label, lo, hi, dlo, dhi);
}

// d Dice / d logit of a row from its rl_dice_row derivatives, the sums A and B over all valid rows and k = upstream gradient x s:
// k * (-dlo / max(B, 1) + [B >= 1] * A / max(B, 1)^2 * dhi); each coefficient is formed in double and rounded to float32 once
RL_FN float rl_dice_grad(float dlo, float dhi, double A, double B, double k) {
    const double Bc = B > 1.0 ? B : 1.0;
    const float c_lo = (float)(-k / Bc);
    const float c_hi = (float)(B >= 1.0 ? k * A / (Bc * Bc) : 0.0);
    return c_lo * dlo + c_hi * dhi;
}

// n-way softmax cross-entropy of logits z[0..n) against `target`; max and log-sum are handed back for the derivative
RL_FN float rl_softmax_ce(const float* z, int n, int target, float* zmax, float* logsum) {
    float m = z[0];
    for (int j = 1; j < n; ++j) m = fmaxf(m, z[j]);
    float s = 0.0f;
    for (int j = 0; j < n; ++j) s = s + expf(z[j] - m);
    const float ls = logf(s);
    *zmax = m;
    *logsum = ls;
    return ls - (z[target] - m);
}

RL_FN float rl_softmax_ce_grad(float zj, float zmax, float logsum, bool is_target) {
    return expf((zj - zmax) - logsum) - (is_target ? 1.0f : 0.0f);
}

RL_FN float rl_smooth_l1(float a, float b, float* da) {
    const float d = a - b;
    const float ad = fabsf(d);
    *da = ad < 1.0f ? d : (d > 0.0f ? 1.0f : -1.0f);
    return ad < 1.0f ? 0.5f * ad * ad : ad - 0.5f;
}

// ---------------------------------------------------------------------------------------------- one foreground row
// one bin head (n logits at z, target t) and one residual head (n columns at z, the target's column against res): the term is
// ADDED to *acc, or with GRAD the columns are overwritten by g * d term / d column
template <bool GRAD, typename ACC>
RL_FN void rl_bin_head(float* z, int n, int t, float g, ACC* acc) {
    float m, ls;
    const float v = rl_softmax_ce(z, n, t, &m, &ls);
    if (GRAD) {
        for (int j = 0; j < n; ++j) z[j] = g * rl_softmax_ce_grad(z[j], m, ls, j == t);
    } else {
        *acc += (ACC)v;
    }
}

template <bool GRAD, typename ACC>
RL_FN void rl_res_head(float* z, int n, int t, float res, float g, ACC* acc) {
    float d;
    const float v = rl_smooth_l1(z[t], res, &d);
    if (GRAD) {
        for (int j = 0; j < n; ++j) z[j] = j == t ? g * d : 0.0f;
    } else {
        *acc += (ACC)v;
    }
}

// row: the C predictions of a foreground row, lab: its 7 labels [dx dy dz h w l ry].  The row's eight regression terms are
// ADDED to acc[RL_X_BIN..RL_SIZE] (the size term as the sum over its three columns); with GRAD the row is overwritten by
// g * d(sum of the row's terms)/d(prediction), the size columns included as they enter the loss (3 * mean over 3 columns).
template <bool GRAD, typename ACC>
RL_FN void rl_reg_row(float* row, const float* lab, const RlConfig& c, float g, ACC* acc) {
    const int nb = c.nb, nh = c.nh;
    int xb, zb, rb;
    float xr, zr, rr;
    rl_bin_and_residual(lab[0], c, &xb, &xr);
    rl_bin_and_residual(lab[2], c, &zb, &zr);
    rl_angle_bin_and_residual(lab[6], c, &rb, &rr);
    int off = 2 * nb;
    rl_bin_head<GRAD>(row, nb, xb, g, &acc[RL_X_BIN]);
    rl_bin_head<GRAD>(row + nb, nb, zb, g, &acc[RL_Z_BIN]);
    if (c.xz_fine) {
        rl_res_head<GRAD>(row + off, nb, xb, xr, g, &acc[RL_X_RES]);
        rl_res_head<GRAD>(row + off + nb, nb, zb, zr, g, &acc[RL_Z_RES]);
        off += 2 * nb;
    }
    rl_res_head<GRAD>(row + off, 1, 0, lab[1], g, &acc[RL_Y_OFF]);
    off += 1;
    rl_bin_head<GRAD>(row + off, nh, rb, g, &acc[RL_RY_BIN]);
    rl_res_head<GRAD>(row + off + nh, nh, rb, rr, g, &acc[RL_RY_RES]);
    off += 2 * nh;
    for (int k = 0; k < 3; ++k) rl_res_head<GRAD>(row + off + k, 1, 0, rl_size_target(lab[3 + k], c.anchor[k]), g, &acc[RL_SIZE]);
}
