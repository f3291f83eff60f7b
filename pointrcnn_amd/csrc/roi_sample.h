// roi_sample.h -- what the two RCNN-stage RoI samplers share, host and device: the online one (proposal_target.hip,
// ProposalTargetLayer.sample_rois_for_rcnn, lib/rpn/proposal_target_layer.py:103-175) and the offline one (rcnn_offline.hip,
// KittiRCNNDataset.get_rcnn_training_sample_batch, lib/datasets/kitti_rcnn_dataset.py:903-957).  Both turn a frame's row maxima into
// three candidate lists, a slot plan and R source RoIs; this header states that selection once, and tests/roi_sample_host.cpp runs it
// on the host against the oracle and the numpy twin.  What differs stays in the kernels: the IoU, how ground truth is counted, the
// labels' best RoIs the offline list ends with, the frame with foreground but no background candidate, and the noise loops.
// The rules the selection carries:
//   the thresholds meet float32 overlaps as float32, the ratios act as Python doubles (RsCfg below);
//   the lists are in RoI order; a row maximum is compared as `>= fg`, `< bg_lo`, `< bg && >= bg_lo`, so a NaN joins no list;
//   sampling without replacement = the places of the foreground list with the smallest (key, place), in that order;
//   a background slot draws below(r, list length) from its own stream, hard slots first.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "counter_rand.h"

// floor(u * n) for u = r / 2^32: np.floor(np.random.rand() * n), np.random.randint(n)
__host__ __device__ __forceinline__ int rs_below(unsigned r, int n) { return (int)(((unsigned long long)r * (unsigned long long)n) >> 32); }

// cfg6 = (REG_FG, CLS_FG, CLS_BG, CLS_BG_LO, FG_RATIO, HARD_BG_RATIO) of both C entry points
struct RsCfg {
    float fg_thresh, cls_bg, cls_bg_lo;
    double pos_thresh, hard_ratio;
    int fg_per_image;
};

inline RsCfg rs_cfg(const double* cfg6, int R) {
    RsCfg c;
    // thresholds meet float32 overlaps (torch casts the Python scalar to the tensor's dtype; numpy compares a float32 ARRAY with a Python
    // float in float32), only the float32 SCALAR of the offline noise loop is compared in double: pos_thresh
    c.pos_thresh = cfg6[0] < cfg6[1] ? cfg6[0] : cfg6[1];
    c.fg_thresh = (float)c.pos_thresh; c.cls_bg = (float)cfg6[2]; c.cls_bg_lo = (float)cfg6[3];
    // the two ratios stay DOUBLE: the reference computes np.round(FG_RATIO * ROI_PER_IMAGE) and int(bg_rois_per_this_image * HARD_BG_RATIO)
    // in Python doubles (0.7f * 10 -> 6, 0.7 * 10 -> 7)
    c.hard_ratio = cfg6[5];
    c.fg_per_image = (int)nearbyint(cfg6[4] * (double)R);                 // np.round
    return c;
}

// one frame's (R) outputs cleared by a workgroup of `step` lanes: src -1, the rest 0
__host__ __device__ inline void rs_clear(float* rois, float* gt_of_rois, float* roi_iou, int32_t* src, int R, int tid, int step) {
    for (int t = tid; t < R; t += step) {
        src[t] = -1; roi_iou[t] = 0.f;
        for (int c = 0; c < 7; c++) { rois[(size_t)t * 7 + c] = 0.f; gt_of_rois[(size_t)t * 7 + c] = 0.f; }
    }
}

struct RsLists { int nfg, nhard, neasy; };

// The candidate lists of n row maxima, in RoI order.  On the device one lane walks this loop (M dependent reads): store and increment
// are written apart because with `fg[nfg++] = i` inside this function hipcc (ROCm 7.2) leaves a scalar copy per append in the loop, which
// measured 2 % of the whole offline call at M = 4096.
__host__ __device__ inline RsLists rs_lists(const float* mo, int n, const RsCfg& c, int* fg, int* hard, int* easy) {
    int nfg = 0, nhard = 0, neasy = 0;
    for (int i = 0; i < n; i++) {
        const float v = mo[i];
        if (v >= c.fg_thresh) { fg[nfg] = i; nfg += 1; }
        if (v < c.cls_bg_lo) { easy[neasy] = i; neasy += 1; }
        if (v < c.cls_bg && v >= c.cls_bg_lo) { hard[nhard] = i; nhard += 1; }
    }
    return {nfg, nhard, neasy};
}

enum { RS_BOTH = 0, RS_FG_ONLY = 1, RS_BG_ONLY = 2, RS_NEITHER = 3 };
struct RsPlan { int kind, fs, bs, nh; };      // foreground slots, background slots, how many of those are hard

// The reference's cases.  RS_FG_ONLY and RS_NEITHER come back without slots: what a frame with foreground but no background candidate
// gets is the caller's (online: all R slots with replacement; offline: the reference raises).
__host__ __device__ inline RsPlan rs_plan(const RsLists& l, int R, int fg_per_image, double hard_ratio) {
    const int nbg = l.nhard + l.neasy;
    RsPlan p = {l.nfg > 0 ? (nbg > 0 ? RS_BOTH : RS_FG_ONLY) : (nbg > 0 ? RS_BG_ONLY : RS_NEITHER), 0, 0, 0};
    if (p.kind == RS_BOTH) { p.fs = fg_per_image < l.nfg ? fg_per_image : l.nfg; p.bs = R - p.fs; }
    else if (p.kind == RS_BG_ONLY) p.bs = R;
    if (l.nhard > 0 && l.neasy > 0) p.nh = (int)((double)p.bs * hard_ratio);
    else if (l.nhard > 0) p.nh = p.bs;
    return p;
}

// without replacement: place t goes to slot rank(t) = the number of places with a smaller (key, place)
__host__ __device__ __forceinline__ int rs_rank(const unsigned* keys, int nfg, int t) {
    const unsigned k = keys[t];
    int rank = 0;
    for (int u = 0; u < nfg; u++) rank += (keys[u] < k || (keys[u] == k && u < t)) ? 1 : 0;
    return rank;
}

// the source RoI of background slot t: the first nh slots draw from the hard list, the others from the easy list
__host__ __device__ __forceinline__ int rs_bg_pick(int t, const RsPlan& p, const RsLists& l, const int* hard, const int* easy, unsigned seed,
                                                   unsigned stream_hard, unsigned stream_easy, unsigned frame) {
    if (t < p.nh) return hard[rs_below(scene_rand(seed, stream_hard, frame, (unsigned)t), l.nhard)];
    return easy[rs_below(scene_rand(seed, stream_easy, frame, (unsigned)(t - p.nh)), l.neasy)];
}

// random_aug_box3d 'multiple': the five [position, size, heading] range rows (proposal_target_layer.py:262-266).  Selects: an indexed
// local table is scratch memory.
struct RsNoiseRange { double pos, hwl, ang; };
__host__ __device__ __forceinline__ RsNoiseRange rs_noise_range(int idx) {
    const double pi = 3.14159265358979323846;
    RsNoiseRange r;
    r.pos = idx == 0 ? 0.2 : idx == 1 ? 0.3 : idx == 2 ? 0.5 : idx == 3 ? 0.8 : 1.0;
    r.hwl = idx == 0 ? 0.1 : 0.15;
    r.ang = idx < 2 ? pi / 12 : idx == 2 ? pi / 9 : idx == 3 ? pi / 6 : pi / 3;
    return r;
}
