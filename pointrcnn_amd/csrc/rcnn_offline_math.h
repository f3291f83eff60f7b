// rcnn_offline_math.h -- the per-slot arithmetic of the RCNN offline sampler (rcnn_offline.hip), host and device.
//
// KittiRCNNDataset.get_rcnn_training_sample_batch (lib/datasets/kitti_rcnn_dataset.py:876-957) measures every box pair with
// kitti_utils.get_iou3d on kitti_utils.boxes3d_to_corners3d corners, and aug_roi_by_noise_batch / random_aug_box3d (:1052-1077,
// :747-788) retry a noisy copy of a sampled RoI until it reaches the foreground threshold.  The rounding points of that code are
// the contract restated here:
//   a float32 box (an input RoI, a label, the keep-the-original branch of the loop): corners in float32 -- local corners
//       x = +-l/2, z = +-w/2, y = 0 / -h, rotated by a (8,3) x (3,3) product, then shifted, with the sine and cosine of ref_trig.h
//       so that host and device give the same bits.  The product has two forms, because numpy's matmul has two: a call on
//       SEVERAL boxes (the M x G matrix) runs numpy's own loop, every operation rounded, summed left to right from zero
//       (ti_corners of train_input.hip); a call on ONE box (the label and the kept original inside the noise loop, or a frame
//       with a single RoI or a single label) has BLAS-compatible strides and goes through sgemm, whose kernel on every
//       FMA-capable x86-64 host accumulates fused: fma(z, sin, x * cos).  The two differ in the last bit for 7 % of all boxes;
//       tests/golden/ref_rcnn_offline.py met both;
//   a noisy box: float32 box + float64 draws = a FLOAT64 box.  boxes3d_to_corners3d stores its local corners in float32 arrays
//       (l/2, w/2 and -h are rounded there), multiplies them by a float64 rotation, adds the float64 centre and rounds the
//       corner to float32 once (kitti_utils.py:74-101).  The stored RoI is the float64 box rounded to float32;
//   the IoU of two corner sets: quad_clip.h.  A separating axis between the two bottoms (the conservative float32 test of
//       train_input.hip) proves that the exact clip is empty: the overlap is then exactly 0 and so is the quotient, the same
//       +0.0f the clip returns, so the test changes no result and only saves the clip;
//   `temp_iou < pos_thresh` compares a numpy float32 scalar with a Python float: in double.
// Randomness: counter_rand.h (through roi_sample.h, whose below() and range rows the online sampler shares), stream RO_STREAM_NOISE, position ((slot * 16 + attempt) * 16 + q) -- q = 8 the keep-the-original
// draw (u < 0.2), q = 0 the range row (below(r, 5)), q = 1..3 position, q = 4..6 size, q = 7 heading.
#pragma once
#include <hip/hip_runtime.h>
#include "quad_clip.h"
#include "roi_sample.h"
#include "ref_trig.h"

constexpr unsigned RO_STREAM_FG_KEY = 40;     // position = place in the foreground list: the draw without replacement
constexpr unsigned RO_STREAM_HARD = 42;       // position = hard-background slot: below(r, list length)
constexpr unsigned RO_STREAM_EASY = 43;       // position = easy-background slot
constexpr unsigned RO_STREAM_NOISE = 50;
constexpr int RO_MAX_AUG_TIMES = 16;          // the attempt field of the noise position is four bits wide

// boxes3d_to_corners3d of a float32 box -> (8,3) float32; fused: the one-box form
__host__ __device__ inline void ro_corners_f32(const float* bx, float* c, bool fused) {
    const float h = bx[3], w = bx[4], l = bx[5];
    const float cs = prcnn_ref_cosf(bx[6]), sn = prcnn_ref_sinf(bx[6]), nsn = -sn;
    const float hl = l / 2.0f, hw = w / 2.0f;
    for (int k = 0; k < 8; ++k) {
        const float xs = (k & 2) ? -hl : hl;
        const float zs = ((k + 1) & 2) ? -hw : hw;
        const float ys = k < 4 ? 0.0f : -h;
        const float xr = fused ? fmaf(zs, sn, fmaf(ys, 0.0f, xs * cs)) : (xs * cs + ys * 0.0f) + zs * sn;
        const float yr = (xs * 0.0f + ys * 1.0f) + zs * 0.0f;             // exact either way
        const float zr = fused ? fmaf(zs, cs, fmaf(ys, 0.0f, xs * nsn)) : (xs * nsn + ys * 0.0f) + zs * cs;
        c[3 * k + 0] = bx[0] + xr;
        c[3 * k + 1] = bx[1] + yr;
        c[3 * k + 2] = bx[2] + zr;
    }
}

// boxes3d_to_corners3d of a float64 box -> (8,3) float32, rounded once
__host__ __device__ inline void ro_corners_f64(const double* bx, float* c) {
    const double cs = cos(bx[6]), sn = sin(bx[6]), nsn = -sn;
    const float hl = (float)(bx[5] / 2.0), hw = (float)(bx[4] / 2.0), nh = (float)(-bx[3]);
    for (int k = 0; k < 8; ++k) {
        const double xs = (k & 2) ? -hl : hl;
        const double zs = ((k + 1) & 2) ? -hw : hw;
        const double ys = k < 4 ? 0.0 : nh;
        const double xr = (xs * cs + ys * 0.0) + zs * sn;
        const double yr = (xs * 0.0 + ys * 1.0) + zs * 0.0;
        const double zr = (xs * nsn + ys * 0.0) + zs * cs;
        c[3 * k + 0] = (float)(bx[0] + xr);
        c[3 * k + 1] = (float)(bx[1] + yr);
        c[3 * k + 2] = (float)(bx[2] + zr);
    }
}

// true when an edge normal of either bottom separates the two bottoms by more than a bound on the float32 rounding of the projections
__host__ __device__ inline bool ro_separated(const float* ca, const float* cb) {
    float S = 1.0f;
    for (int k = 0; k < 4; ++k)
        S = fmaxf(S, fmaxf(fmaxf(fabsf(ca[3 * k]), fabsf(ca[3 * k + 2])), fmaxf(fabsf(cb[3 * k]), fabsf(cb[3 * k + 2]))));
    for (int e = 0; e < 8; ++e) {
        const float* q = e < 4 ? ca : cb;
        const int i = e & 3, j = (i + 1) & 3;
        const float nx = -(q[3 * j + 2] - q[3 * i + 2]), nz = q[3 * j] - q[3 * i];
        const float margin = 1e-5f * (fabsf(nx) + fabsf(nz)) * S;
        float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
        for (int k = 0; k < 4; ++k) {
            const float pa = ca[3 * k] * nx + ca[3 * k + 2] * nz, pb = cb[3 * k] * nx + cb[3 * k + 2] * nz;
            amin = fminf(amin, pa); amax = fmaxf(amax, pa);
            bmin = fminf(bmin, pb); bmax = fmaxf(bmax, pb);
        }
        if (amax < bmin - margin || bmax < amin - margin) return true;
    }
    return false;
}

// get_iou3d for one pair of corner sets
__host__ __device__ inline float ro_pair_iou(const float* ca, const float* cb) {
    float lo_a, hi_a, lo_b, hi_b;
    qc_heights(ca, lo_a, hi_a);
    qc_heights(cb, lo_b, hi_b);
    const float h = qc_h_overlap(lo_a, hi_a, lo_b, hi_b);
    if (h == 0.0f || ro_separated(ca, cb)) return 0.0f;
    const QcQuad qa = qc_make(ca), qb = qc_make(cb);
    float v3, vb;
    qc_ratios(qa, qb, h, hi_a - lo_a, hi_b - lo_b, v3, vb);
    return v3;
}

// random_aug_box3d: method 0 'multiple' (:760-774), 1 'single' (:752-759); base = the attempt's first position
__host__ __device__ inline void ro_noise_box(const float* box, unsigned seed, unsigned frame, unsigned base, int method, double* aug) {
    const double pi = 3.14159265358979323846;
    const RsNoiseRange rg = rs_noise_range(method == 0 ? rs_below(scene_rand(seed, RO_STREAM_NOISE, frame, base), 5) : 0);      // roi_sample.h
    for (int c = 0; c < 3; ++c) {
        const double up = scene_u01(scene_rand(seed, RO_STREAM_NOISE, frame, base + 1 + c)) - 0.5;
        const double uh = scene_u01(scene_rand(seed, RO_STREAM_NOISE, frame, base + 4 + c)) - 0.5;
        const double ps = method == 0 ? (up / 0.5) * rg.pos : up;
        const double hs = method == 0 ? (uh / 0.5) * rg.hwl + 1.0 : uh / (0.5 / 0.15) + 1.0;
        aug[c] = (double)box[c] + ps;
        aug[3 + c] = (double)box[3 + c] * hs;
    }
    const double ua = scene_u01(scene_rand(seed, RO_STREAM_NOISE, frame, base + 7)) - 0.5;
    aug[6] = (double)box[6] + (method == 0 ? (ua / 0.5) * rg.ang : ua / (0.5 / (pi / 12)));
}

// aug_roi_by_noise_batch for one slot: box = the sampled RoI, gtc = its label's corners (one-box form), times = 10 (foreground) / 1 (background).
// -> roi (7) the loop's last box as float32, *iou the loop's last IoU (0 when the loop did not run); returns the attempts made
__host__ __device__ inline int ro_noise_slot(const float* box, const float* gtc, int times, double pos_thresh, unsigned seed, unsigned frame,
                                             unsigned slot, int method, float* roi, float* iou) {
    float temp_iou = 0.0f;
    int cnt = 0;
    for (int c = 0; c < 7; ++c) roi[c] = box[c];
    while ((double)temp_iou < pos_thresh && cnt < times) {
        const unsigned base = (slot * 16u + (unsigned)cnt) * 16u;
        float cr[24];
        if (scene_u01(scene_rand(seed, RO_STREAM_NOISE, frame, base + 8)) < 0.2) {
            for (int c = 0; c < 7; ++c) roi[c] = box[c];
            ro_corners_f32(box, cr, true);
        } else {
            double aug[7];
            ro_noise_box(box, seed, frame, base, method, aug);
            ro_corners_f64(aug, cr);
            for (int c = 0; c < 7; ++c) roi[c] = (float)aug[c];
        }
        temp_iou = ro_pair_iou(cr, gtc);
        ++cnt;
    }
    *iou = temp_iou;
    return cnt;
}

// ------------------------------------------------------------------------------------------------ after pooling
// The rest of get_rcnn_training_sample_batch (:976-1010) for one slot: data_augmentation(mustaug=True, stage=2) (:513-570) with
// rotate_box3d_along_y (:396-406), then canonical_transform_batch (:685-704) and the labels (:998-1007).  Rounding points:
//   rotation of points and box centres: rotate_pc_along_y, a float32-by-float64 np.dot stored to float32 --
//       x' = f32(x * cos + z * (-sin)), z' = f32(x * sin + z * cos) with the double sine / cosine of the drawn angle;
//   a box's ry: beta = atan2f(z, x) (ref_trig.h), alpha = ((-sign(beta) * pi) / 2 + beta) + ry, after the rotation
//       ry = ((sign(beta') * pi) / 2 + alpha) - beta', every operation a float32 one with pi = float32(pi);
//   scale: a float32 product with float32(scale) on the points and on the boxes' first six fields;
//   flip: x = -x, ry = sign(ry) * pi - ry in float32;
//   canonical transform: ry mod 2 pi with numpy's float32 remainder, the centre subtracted in float32, then torch's float32
//       rotation x' = x * cos + z * (-sin), z' = x * sin + z * cos (cosine / sine of ref_trig.h, every operation rounded);
//       gt_boxes3d_ct is the label moved the same way with ry - (RoI ry mod 2 pi).
// Randomness: stream 51 position slot * 4 + i, i = 0..2: aug_enable = 1 - u01 (mustaug overrides i = 0, 1: rotation and scale always
// run, the flip runs iff 1 - u01 < AUG_METHOD_PROB[2]); stream 52 position slot: angle = lo + (hi - lo) * u01 over +-pi / AUG_ROT_RANGE;
// stream 53 position slot: scale = 0.95 + (1.05 - 0.95) * u01.
constexpr unsigned RO_STREAM_AUG_ENABLE = 51, RO_STREAM_AUG_ANGLE = 52, RO_STREAM_AUG_SCALE = 53;
#define RO_PI_F 3.14159274101257324f

struct RoAug {
    int rot, scl, flip;
    double cs, sn;          // of the drawn angle
    float scale;
};

// methods: bit 0 'rotation', bit 1 'scaling', bit 2 'flip' in AUG_METHOD_LIST (0: AUG_DATA off)
__host__ __device__ inline RoAug ro_aug_draw(unsigned seed, unsigned frame, unsigned slot, int methods, double flip_prob, double rot_range) {
    RoAug a;
    a.rot = methods & 1; a.scl = (methods >> 1) & 1; a.cs = 1.0; a.sn = 0.0; a.scale = 1.0f;
    a.flip = (methods & 4) && (1.0 - scene_u01(scene_rand(seed, RO_STREAM_AUG_ENABLE, frame, slot * 4u + 2u)) < flip_prob);
    if (a.rot) {
        const double pi = 3.14159265358979323846, lo = -pi / rot_range, hi = pi / rot_range;
        const double angle = lo + (hi - lo) * scene_u01(scene_rand(seed, RO_STREAM_AUG_ANGLE, frame, slot));
        a.cs = cos(angle); a.sn = sin(angle);
    }
    if (a.scl) a.scale = (float)(0.95 + (1.05 - 0.95) * scene_u01(scene_rand(seed, RO_STREAM_AUG_SCALE, frame, slot)));
    return a;
}

__host__ __device__ __forceinline__ float ro_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }

__host__ __device__ __forceinline__ void ro_rotate_f64(float* x, float* z, double cs, double sn) {
    const double xd = *x, zd = *z;
    *x = (float)(xd * cs + zd * (-sn));
    *z = (float)(xd * sn + zd * cs);
}

// data_augmentation(stage=2) on one point
__host__ __device__ __forceinline__ void ro_aug_point(float* p, const RoAug& a) {
    if (a.rot) ro_rotate_f64(&p[0], &p[2], a.cs, a.sn);
    if (a.scl) { p[0] = p[0] * a.scale; p[1] = p[1] * a.scale; p[2] = p[2] * a.scale; }
    if (a.flip) p[0] = -p[0];
}

// ... and on one box (rotate_box3d_along_y, :396-406)
__host__ __device__ inline void ro_aug_box(float* b, const RoAug& a) {
    if (a.rot) {
        const float beta = prcnn_ref_atan2f(b[2], b[0]);
        const float alpha = ((-ro_sign(beta) * RO_PI_F) / 2.0f + beta) + b[6];
        ro_rotate_f64(&b[0], &b[2], a.cs, a.sn);
        const float nb = prcnn_ref_atan2f(b[2], b[0]);
        b[6] = ((ro_sign(nb) * RO_PI_F) / 2.0f + alpha) - nb;
    }
    if (a.scl)
        for (int c = 0; c < 6; ++c) b[c] = b[c] * a.scale;
    if (a.flip) {
        b[0] = -b[0];
        b[6] = ro_sign(b[6]) * RO_PI_F - b[6];
    }
}

struct RoCanon { float cx, cy, cz, ry, cs, sn; };

// numpy's float32 remainder by float32(2 pi)
__host__ __device__ inline RoCanon ro_canon_of(const float* roi) {
    RoCanon c;
    const float two_pi = 6.28318548202514648f;
    float r = fmodf(roi[6], two_pi);
    if (r != 0.0f && r < 0.0f) r += two_pi;
    c.cx = roi[0]; c.cy = roi[1]; c.cz = roi[2]; c.ry = r;
    c.cs = prcnn_ref_cosf(r); c.sn = prcnn_ref_sinf(r);
    return c;
}

__host__ __device__ __forceinline__ void ro_canon_point(float* p, const RoCanon& c) {
    const float x = p[0] - c.cx, y = p[1] - c.cy, z = p[2] - c.cz;
    p[0] = x * c.cs + z * (-c.sn);
    p[1] = y;
    p[2] = x * c.sn + z * c.cs;
}

// the slot's boxes: roi and gt are augmented in place, ct receives gt_boxes3d_ct; -> the canonical frame of the augmented RoI
__host__ __device__ inline RoCanon ro_finish_boxes(float* roi, float* gt, const RoAug& a, float* ct) {
    ro_aug_box(roi, a);
    ro_aug_box(gt, a);
    const RoCanon c = ro_canon_of(roi);
    for (int q = 0; q < 7; ++q) ct[q] = gt[q];
    ro_canon_point(ct, c);
    ct[6] = gt[6] - c.ry;
    return c;
}

// :998-1007: -> cls_label in {-1, 0, 1}, *mask = reg_valid_mask; thresholds as float32 (array compares)
__host__ __device__ __forceinline__ int ro_labels(float iou, int empty, float reg_fg, float cls_fg, float cls_bg, int* mask) {
    const int valid = empty == 0;
    *mask = (iou > reg_fg) && valid;
    int label = iou > cls_fg;
    if (iou > cls_bg && iou < cls_fg) label = -1;
    if (!valid) label = -1;
    return label;
}
