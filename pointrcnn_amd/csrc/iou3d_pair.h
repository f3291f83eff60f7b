// iou3d_pair.h -- the 3-D IoU of one box pair, iou3d_utils.boxes_iou3d_gpu (lib/utils/iou3d/iou3d_utils.py:20-53) for one entry of its
// matrix: the arithmetic behind prcnn_boxes_iou3d, shared by proposal_target.hip (RoI sampling, the IoU matrix) and eval_stats.hip
// (per-ground-truth maximum IoU of the evaluation loops), and live_gt, how both count a frame's padded ground truth.  One definition:
// both units compute the same bits.
//
// iou3d_pair_s takes the storage of the clip's point list as iou_bev_s does (iou3d_geom.h: ClipPrivate = thread-local arrays, which
// live in scratch memory; ClipLds = a lane-private LDS column) -- same operations in the same order, same bits either way.
#pragma once
#include "iou3d_geom.h"

__device__ __forceinline__ void bev_of(const float* b, float* o) {                  // kitti_utils.py:134-147
    o[0] = sub(b[0], b[5] / 2); o[1] = sub(b[2], b[4] / 2); o[2] = add(b[0], b[5] / 2); o[3] = add(b[2], b[4] / 2); o[4] = b[6];
}

// The ground truth of a frame without its all-zero rows at the end (proposal_target_layer.py:96-99); `keep` rows always stay: 0 for the
// sampler and for eval_rcnn.py:541-548 (`while tmp_idx >= 0`), 1 for :183-186 (`while k > 0`: row 0 stays even when it is all zero)
__device__ __forceinline__ int live_gt(const float* gt, int G, int gt_cols, int keep) {
    int ng = G;
    while (ng > keep) {
        float s = 0.f;
        for (int c = 0; c < gt_cols; c++) s = add(s, gt[(size_t)(ng - 1) * gt_cols + c]);
        if (s != 0.f) break;
        ng--;
    }
    return ng;
}

// iou3d_utils.py:20-53 for one pair; B: the ground-truth box with its RBox already built
template <class S>
__device__ __forceinline__ float iou3d_pair_s(const float* a, const float* b, const RBox& rb, S& st) {
    float abev[5];
    bev_of(a, abev);
    RBox ra;
    make_rbox(abev, ra);
    const float ov = far_apart(ra, rb) ? 0.0f : box_overlap_s(ra, rb, st);
    const float amin = sub(a[1], a[3]), bmin = sub(b[1], b[3]);
    const float max_of_min = amin > bmin ? amin : bmin, min_of_max = a[1] < b[1] ? a[1] : b[1];
    float h = sub(min_of_max, max_of_min);
    if (!(h > 0.0f)) h = 0.0f;
    const float ov3 = mul(ov, h);
    const float va = mul(mul(a[3], a[4]), a[5]), vb = mul(mul(b[3], b[4]), b[5]);
    float den = sub(add(va, vb), ov3);
    if (den < 1e-7f) den = 1e-7f;
    return ov3 / den;
}
__device__ float iou3d_pair(const float* a, const float* b, const RBox& rb) { ClipPrivate st; return iou3d_pair_s(a, b, rb, st); }
