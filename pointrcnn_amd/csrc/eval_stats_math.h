// eval_stats_math.h -- the per-item arithmetic of the evaluation statistics (tools/eval_rcnn.py: eval_one_epoch_rpn :171-202,
// eval_one_epoch_rcnn :336-364, eval_one_epoch_joint :539-573), for host and device (eval_stats.hip; the host build is
// tests/eval_stats_math_host.cpp).
//
// Recall: `(gt_max_iou > thresh).sum()` for thresh in [0.1, 0.3, 0.5, 0.7, 0.9] (:193-194, :343-352, :555-566).  torch compares a float32
// tensor with a Python double in float32 (the scalar is rounded first): float32(0.1) itself is NOT recalled at 0.1 although it is the
// larger number.  A NaN maximum (torch.max propagates it) and the -1 written past a frame's live boxes are never recalled.
// Segmentation IoU (:198-202, :568-573): correct = #(seg == label and label > 0), union = #(label > 0) + #(seg > 0) - correct, both
// integers (the reference forms them in float32, exact below 2^24), then float32(correct) / max(float32(union), 1) in float32.
// RCNN classification accuracy (:355-364), float32: label = gt_iou > fg, valid = gt_iou >= fg or gt_iou <= bg,
// acc = sum((pred == label) * valid) / max(sum(valid), 1), acc_refined = #(pred == (gt_iou >= thr)) / max(R, 1).
// Every ratio is widened to double (`.item()`) and added to a Python float: EsState::sums, in the reference's order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ES_FN __host__ __device__ __forceinline__

constexpr int ES_THRESHOLDS = 5;
constexpr int ES_COUNTERS = 16, ES_SUMS = 4;
// counters: [0..4] ground-truth boxes recalled by set 0 (the RoIs) at the five thresholds, [5..9] by set 1 (the refined boxes)
enum { ES_RECALL0 = 0, ES_RECALL1 = 5, ES_GT = 10, ES_DET = 11, ES_FRAMES = 12, ES_BATCHES = 13 };
enum { ES_SUM_SEG_IOU = 0, ES_SUM_CLS_ACC = 1, ES_SUM_CLS_ACC_REFINED = 2 };

struct EsState {                              // the caller's persistent state: 160 bytes, zeroed by reset
    int64_t counters[ES_COUNTERS];
    double sums[ES_SUMS];
};

struct EsBatch {                              // what one accumulate call reads; every optional group null when absent
    const float* gt_max;                      // (S, B, G), -1 past num_gt[b]
    const int32_t* num_gt;                    // (B)
    int S, B, G;
    const int32_t* det_num;                   // (B) or null
    const float* seg;                         // (B, N) 0 / 1, or null
    const void* cls_label;                    // (B, N) i32 or i64
    int label_is_i64, seg_mode;               // seg_mode 0: one ratio per frame; 1: the batch's ratio added once per frame
    int64_t N;
    const uint8_t* pred_class;                // (B, R) 0 / 1, or null
    const float* gt_iou;                      // (B, R)
    int R;
    float cls_fg, cls_bg, refine_thresh;      // CLS_FG_THRESH, CLS_BG_THRESH, 0.7 for Car / 0.5 otherwise -- rounded to float32 once
};

ES_FN float es_threshold(int t) {             // float32 of the Python doubles 0.1 0.3 0.5 0.7 0.9
    return t == 0 ? 0.1f : t == 1 ? 0.3f : t == 2 ? 0.5f : t == 3 ? 0.7f : 0.9f;
}
ES_FN bool es_recalled(float gt_max, int t) { return gt_max > es_threshold(t); }

ES_FN int64_t es_label_at(const void* lab, int is_i64, int64_t i) {
    return is_i64 ? static_cast<const int64_t*>(lab)[i] : (int64_t)static_cast<const int32_t*>(lab)[i];
}
// one point of the segmentation IoU: bit 0 correct, bit 1 foreground label, bit 2 predicted foreground
ES_FN int es_seg_point(float seg, int64_t label) {
    const bool fg = label > 0, pos = seg > 0.0f;
    const bool same = seg == (float)label;    // seg_result == rpn_cls_label; seg is 0 / 1, so no cast of a float to an integer is needed
    return (same && fg ? 1 : 0) | (fg ? 2 : 0) | (pos ? 4 : 0);
}
ES_FN float es_ratio(int64_t num, int64_t den) {          // float32(num) / max(float32(den), 1), one float32 division
    const float d = (float)den;
    return (float)num / (d > 1.0f ? d : 1.0f);
}
ES_FN float es_seg_iou(int64_t correct, int64_t fg, int64_t pos) { return es_ratio(correct, fg + pos - correct); }

// one RoI of the classification accuracy: bit 0 (pred == label) and valid, bit 1 valid, bit 2 pred == refined label
ES_FN int es_cls_roi(int pred, float gt_iou, float fg, float bg, float refine_thresh) {
    const int label = gt_iou > fg ? 1 : 0;
    const bool valid = gt_iou >= fg || gt_iou <= bg;
    const int refined = gt_iou >= refine_thresh ? 1 : 0;
    return ((pred == label) && valid ? 1 : 0) | (valid ? 2 : 0) | (pred == refined ? 4 : 0);
}

// The whole accumulate step, serially: what es_accumulate_kernel computes with one workgroup (integer counts in any order, the double
// sums by one thread in this order).
static inline void es_accumulate_serial(const EsBatch& P, EsState* st) {
    for (int s = 0; s < P.S && P.G > 0; ++s)
        for (int b = 0; b < P.B; ++b)
            for (int j = 0; j < P.num_gt[b]; ++j)
                for (int t = 0; t < ES_THRESHOLDS; ++t)
                    st->counters[(s ? ES_RECALL1 : ES_RECALL0) + t] += es_recalled(P.gt_max[((size_t)s * P.B + b) * P.G + j], t) ? 1 : 0;
    for (int b = 0; b < P.B; ++b) {
        if (P.G > 0) st->counters[ES_GT] += P.num_gt[b];
        if (P.det_num) st->counters[ES_DET] += P.det_num[b];
    }
    st->counters[ES_FRAMES] += P.B;
    st->counters[ES_BATCHES] += 1;
    if (P.seg) {
        int64_t all[3] = {0, 0, 0};
        for (int b = 0; b < P.B; ++b) {
            int64_t c[3] = {0, 0, 0};
            for (int64_t i = 0; i < P.N; ++i) {
                const int bits = es_seg_point(P.seg[b * P.N + i], es_label_at(P.cls_label, P.label_is_i64, b * P.N + i));
                for (int q = 0; q < 3; ++q) c[q] += (bits >> q) & 1;
            }
            if (P.seg_mode == 0) st->sums[ES_SUM_SEG_IOU] += (double)es_seg_iou(c[0], c[1], c[2]);
            for (int q = 0; q < 3; ++q) all[q] += c[q];
        }
        if (P.seg_mode == 1)                  // eval_rcnn.py:568-573 sits inside `for k in range(batch_size)`: B additions of the batch's ratio
            for (int b = 0; b < P.B; ++b) st->sums[ES_SUM_SEG_IOU] += (double)es_seg_iou(all[0], all[1], all[2]);
    }
    if (P.pred_class)
        for (int b = 0; b < P.B; ++b) {
            int64_t c[3] = {0, 0, 0};
            for (int r = 0; r < P.R; ++r) {
                const int bits = es_cls_roi(P.pred_class[(size_t)b * P.R + r], P.gt_iou[(size_t)b * P.R + r], P.cls_fg, P.cls_bg, P.refine_thresh);
                for (int q = 0; q < 3; ++q) c[q] += (bits >> q) & 1;
            }
            st->sums[ES_SUM_CLS_ACC] += (double)es_ratio(c[0], c[1]);
            st->sums[ES_SUM_CLS_ACC_REFINED] += (double)es_ratio(c[2], P.R);
        }
}
