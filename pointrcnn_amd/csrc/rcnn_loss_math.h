// rcnn_loss_math.h -- what the RCNN training loss (pointrcnn_amd/train_functions.py get_rcnn_loss, i.e. lib/net/train_functions.py:122-214
// with get_reg_loss(get_xz_fine=True, get_ry_fine=True)) adds to the arithmetic of rpn_loss_math.h, for one row, for host and device
// (rcnn_loss.hip; the host build is tests/rcnn_loss_math_host.cpp).  rl_focal, rl_softmax_ce, rl_smooth_l1, rl_bin_head, rl_res_head
// and rl_bin_and_residual are used as they are.
//
// Label targets -- the contract of rpn_loss_math.h: torch's CPU float32 sequence bit for bit, every Python double constant rounded to
// float32 once on the host (rc_make_config), every operation individually rounded, `%` as torch.remainder, bins clamped into range.
//   fine angle (get_ry_fine=True): ry = ry % 2pi; if (ry > pi/2) & (ry < 3pi/2): ry = (ry + pi) % 2pi;
//                       shift = clamp(((ry + pi/2) % 2pi) - pi/4, 1e-3, pi/2 - 1e-3); apc = (pi/2) / num_head_bin;
//                       bin = clamp(floor(shift / apc), 0, num_head_bin - 1); res = (shift - (float(bin) * apc + apc/2)) / (apc/2)
//     torch compares a float32 tensor with a Python double in float32 (the scalar is rounded first): float32(pi/2) itself is NOT
//     "> math.pi * 0.5" although it is the larger number.  The comparisons below are float32 against the rounded constants.
//     A NaN angle fails both comparisons, passes through the clamp as NaN (torch.clamp propagates it) and lands in bin 0.
//   y bin head (get_y_by_bin):  _bin_and_residual with LOC_Y_SCOPE / LOC_Y_BIN_SIZE (rl_bin_and_residual on RcConfig::y)
//   size:               (hwl - anchor) / anchor, the anchor MEAN_SIZE or the row's own roi_boxes3d[3:6] (SIZE_RES_ON_ROI)
//
// Binary cross-entropy of one row, F.binary_cross_entropy(sigmoid(x), t) with t = max(label, 0) in {0, 1} (its log is clamped at -100):
//   value  min(softplus(-x), 100) * t + min(softplus(x), 100) * (1 - t),  softplus(z) = max(z, 0) + log1p(exp(-|z|))
//   d/dx   p - t, formed without cancellation: sigmoid(x) for t = 0, -sigmoid(-x) for t = 1
// Where the clamp at 100 is active (x > 100 against t = 0, x < -100 against t = 1) the value is 100 and the derivative stays p - t
// (+-1 there): the gradient of the unclamped term, magnitude <= 1 everywhere.  The composed float32 code returns 0 there, and already
// from |x| ~ 17 on, where float32 sigmoid(x) rounds to 1 and its log to -inf; float64 keeps p - t up to |x| ~ 37.
#pragma once
#include "rpn_loss_math.h"

constexpr int RC_TERMS = 12;              // per-row sums: cls cls_pos cls_neg x_bin z_bin x_res z_res y(offset | bin) y_res ry_bin ry_res size
enum { RC_CLS = 0, RC_CLS_POS, RC_CLS_NEG, RC_X_BIN, RC_Z_BIN, RC_X_RES, RC_Z_RES, RC_Y_A, RC_Y_RES, RC_RY_BIN, RC_RY_RES, RC_SIZE };
constexpr int RC_LOSS_FOCAL = 0, RC_LOSS_BCE = 2;      // ops.rpn_loss_cfg's numbering

struct RcConfig {
    RlConfig xz;                              // x / z heads, focal parameters (rl_make_config; its angle fields are the coarse ones, unused)
    RlConfig y;                               // y bin head: scope, shift_hi, bin, half_bin, nb of LOC_Y_SCOPE / LOC_Y_BIN_SIZE; the rest unused
    float two_pi, pi, half_pi, three_half_pi, quarter_pi;      // 2pi, pi, pi*0.5, pi*1.5, pi*0.25
    float shift_lo, shift_hi;                 // 1e-3, pi*0.5 - 1e-3
    float apc, half_apc;                      // (pi/2) / num_head_bin and half of it
    int nh, y_by_bin, size_on_roi, loss_cls;  // angle bins, LOC_Y_BY_BIN, SIZE_RES_ON_ROI, RC_LOSS_*
    int C;                                    // channels of a regression row: 4 nb + (2 nby | 1) + 2 nh + 3
};

static inline RcConfig rc_make_config(double loc_scope, double loc_bin_size, int num_head_bin, int y_by_bin, double loc_y_scope,
                                      double loc_y_bin_size, int size_on_roi, const double* mean_size, int loss_cls, double gamma,
                                      double alpha, int has_alpha) {
    RcConfig c;
    const double pi = 3.141592653589793;
    const double apc = (pi / 2) / num_head_bin;
    c.xz = rl_make_config(loc_scope, loc_bin_size, num_head_bin, 1, mean_size, gamma, alpha, has_alpha, 1.0, 1.0);
    c.y = rl_make_config(loc_y_scope, loc_y_bin_size, num_head_bin, 1, mean_size, gamma, alpha, has_alpha, 1.0, 1.0);
    c.two_pi = (float)(2 * pi);
    c.pi = (float)pi;
    c.half_pi = (float)(pi * 0.5);
    c.three_half_pi = (float)(pi * 1.5);
    c.quarter_pi = (float)(pi * 0.25);
    c.shift_lo = (float)1e-3;
    c.shift_hi = (float)(pi * 0.5 - 1e-3);
    c.apc = (float)apc;
    c.half_apc = (float)(apc / 2);
    c.nh = num_head_bin;
    c.y_by_bin = y_by_bin;
    c.size_on_roi = size_on_roi;
    c.loss_cls = loss_cls;
    c.C = 4 * c.xz.nb + (y_by_bin ? 2 * c.y.nb : 1) + 2 * num_head_bin + 3;
    return c;
}

// ---------------------------------------------------------------------------------------------- label targets (bitwise contract)
RL_FN void rc_fine_angle_bin_and_residual(float ry, const RcConfig& c, int* bin, float* res) {
    ry = rl_remainder(ry, c.two_pi);
    if (ry > c.half_pi && ry < c.three_half_pi) ry = rl_remainder(ry + c.pi, c.two_pi);
    float s = rl_remainder(ry + c.half_pi, c.two_pi) - c.quarter_pi;
    s = s < c.shift_lo ? c.shift_lo : s;                       // a NaN stays a NaN, as in torch.clamp
    s = s > c.shift_hi ? c.shift_hi : s;
    const int b = rl_bin_index(floorf(s / c.apc), c.nh);
    *bin = b;
    *res = (s - ((float)b * c.apc + c.half_apc)) / c.half_apc;
}

// ---------------------------------------------------------------------------------------------- per-row terms
// BCE term of one row with target t in {0, 1} and its derivative in the logit (the header comment: clamp at 100)
RL_FN void rc_bce(float x, float t, float* val, float* dx) {
    const float e = expf(-fabsf(x));
    const float l = log1pf(e);
    const float sp_pos = fminf(fmaxf(x, 0.0f) + l, 100.0f);    // softplus(x)  = -log(1 - p)
    const float sp_neg = fminf(fmaxf(-x, 0.0f) + l, 100.0f);   // softplus(-x) = -log(p)
    const float big = 1.0f / (1.0f + e), small = e / (1.0f + e);      // sigmoid(|x|), sigmoid(-|x|)
    *val = t > 0.0f ? sp_neg : sp_pos;
    *dx = t > 0.0f ? -(x >= 0.0f ? small : big) : (x >= 0.0f ? big : small);
}

// row: the C predictions of a row whose reg_valid_mask is set, lab: gt_of_rois [dx dy dz h w l ry], anchor: the 3 sizes the size
// target is taken against.  The row's nine regression terms are ADDED to acc[RC_X_BIN..RC_SIZE] (the size term as the sum over its
// three columns); with GRAD the row is overwritten by g * d(sum of the row's terms)/d(prediction), as rl_reg_row.
template <bool GRAD, typename ACC>
RL_FN void rc_reg_row(float* row, const float* lab, const float* anchor, const RcConfig& c, float g, ACC* acc) {
    const int nb = c.xz.nb, nh = c.nh;
    int xb, zb, rb;
    float xr, zr, rr;
    rl_bin_and_residual(lab[0], c.xz, &xb, &xr);
    rl_bin_and_residual(lab[2], c.xz, &zb, &zr);
    rc_fine_angle_bin_and_residual(lab[6], c, &rb, &rr);
    rl_bin_head<GRAD>(row, nb, xb, g, &acc[RC_X_BIN]);
    rl_bin_head<GRAD>(row + nb, nb, zb, g, &acc[RC_Z_BIN]);
    rl_res_head<GRAD>(row + 2 * nb, nb, xb, xr, g, &acc[RC_X_RES]);
    rl_res_head<GRAD>(row + 3 * nb, nb, zb, zr, g, &acc[RC_Z_RES]);
    int off = 4 * nb;
    if (c.y_by_bin) {
        int yb;
        float yr;
        rl_bin_and_residual(lab[1], c.y, &yb, &yr);
        rl_bin_head<GRAD>(row + off, c.y.nb, yb, g, &acc[RC_Y_A]);
        rl_res_head<GRAD>(row + off + c.y.nb, c.y.nb, yb, yr, g, &acc[RC_Y_RES]);
        off += 2 * c.y.nb;
    } else {
        rl_res_head<GRAD>(row + off, 1, 0, lab[1], g, &acc[RC_Y_A]);
        off += 1;
    }
    rl_bin_head<GRAD>(row + off, nh, rb, g, &acc[RC_RY_BIN]);
    rl_res_head<GRAD>(row + off + nh, nh, rb, rr, g, &acc[RC_RY_RES]);
    off += 2 * nh;
    for (int k = 0; k < 3; ++k) rl_res_head<GRAD>(row + off + k, 1, 0, rl_size_target(lab[3 + k], anchor[k]), g, &acc[RC_SIZE]);
}
