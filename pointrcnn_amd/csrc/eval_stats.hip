// eval_stats.hip -- the numbers tools/eval_rcnn.py reports next to the AP, counted on the device: recall of the ground truth by the RoIs
// and by the refined boxes at five IoU thresholds, segmentation IoU, RCNN classification accuracy, detections per frame
// (eval_one_epoch_rpn :171-202, eval_one_epoch_rcnn :336-364, eval_one_epoch_joint :539-573).  The reference walks the batch in a Python
// loop: per frame two (M x G) IoU matrices, a max, five compares and eleven or more `.item()` reads.  Here a batch is two launches and
// nothing returns to the host.
//
//   es_gt_max_kernel      one wave per (box set, frame, ground-truth box): the box's RBox built once, 64 lanes striding over the M
//                         predicted boxes with iou3d_pair_s (the arithmetic of prcnn_boxes_iou3d; every pair runs the full clip), the
//                         clip's point list in a lane-private LDS column (no scratch), shuffle tree for the maximum, ballot for the NaN
//                         flag: torch.max(dim=0) returns NaN when any IoU of the column is NaN, a float `max` would drop it.
//                         Both box sets (RoIs, refined boxes) in one launch.  The other mapping at hand -- pt_overlaps_kernel's 4 RoIs x
//                         16 lanes per wave -- was not measured against this one.
//   es_accumulate_kernel  ONE workgroup, launched in stream order, the only writer of the caller's state: integer counts through LDS,
//                         the float32 ratios widened to double and added by one thread in the reference's order (frame by frame), so
//                         two runs give identical bytes.  No float atomics, no cross-workgroup protocol.
#include "iou3d_pair.h"
#include "eval_stats_math.h"

#define ES_MAX_GT 128
#define ES_ACC_THREADS 1024

struct EsGtMaxParams {
    const float* boxes0;     // (B, M, 7) set 0
    const float* boxes1;     // (B, M, 7) set 1 (S == 2)
    const float* gt;         // (B, G, gt_cols)
    int S, B, M, G, gt_cols, trim_mode;
    float* gt_max;           // (S, B, G)
    int32_t* num_gt;         // (B)
};

__global__ __launch_bounds__(64) void es_gt_max_kernel(const EsGtMaxParams P) {
    __shared__ float s_clip[CLIP_LDS_FLOATS * 64];
    const int j = blockIdx.x, b = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
    const float* gt = P.gt + (size_t)b * P.G * P.gt_cols;
    const int ng = live_gt(gt, P.G, P.gt_cols, P.trim_mode);      // iou3d_pair.h; trim_mode = the rows that always stay
    float* out = P.gt_max + ((size_t)s * P.B + b) * P.G + j;
    if (s == 0 && j == 0 && lane == 0) P.num_gt[b] = ng;
    if (j >= ng) {                                       // every output byte is defined
        if (lane == 0) *out = -1.0f;
        return;
    }
    float g[7], bev[5];
    RBox rb;
    for (int c = 0; c < 7; c++) g[c] = gt[(size_t)j * P.gt_cols + c];
    bev_of(g, bev);
    make_rbox(bev, rb);
    const float* boxes = (s == 0 ? P.boxes0 : P.boxes1) + (size_t)b * P.M * 7;
    ClipLds st;
    st.b = s_clip + lane;
    st.T = 64;
    float best = -INFINITY;
    bool nan = false;
    for (int i = lane; i < P.M; i += 64) {
        float a[7];
        for (int c = 0; c < 7; c++) a[c] = boxes[(size_t)i * 7 + c];
        const float v = iou3d_pair_s(a, g, rb, st);
        if (v != v) nan = true;
        else if (v > best) best = v;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        if (ob > best) best = ob;
    }
    const bool any_nan = __ballot(nan) != 0;
    if (lane == 0) *out = any_nan ? __builtin_nanf("") : best;
}

PRCNN_API size_t prcnn_eval_stats_workspace_bytes(int S, int B, int G) {
    if (S < 0 || B < 0 || G < 0) return 0;
    return (((size_t)S * B * G + (size_t)B) * 4 + 7) & ~(size_t)7;
}

PRCNN_API int prcnn_eval_gt_max_iou(const float* boxes0, const float* boxes1, int S, int B, int M, const float* gt_boxes3d, int G, int gt_cols,
                                    int trim_mode, float* gt_max, int32_t* num_gt, prcnn_stream_t stream) {
    PRCNN_REQUIRE((S == 1 || S == 2) && B >= 0 && B <= 65535 && M >= 1 && G >= 1 && G <= ES_MAX_GT && gt_cols >= 7,
                  "prcnn_eval_gt_max_iou: bad shape S=%d (1 | 2) B=%d M=%d (>= 1) G=%d (1..%d) gt_cols=%d (>= 7)", S, B, M, G, ES_MAX_GT, gt_cols);
    PRCNN_REQUIRE(trim_mode == 0 || trim_mode == 1, "prcnn_eval_gt_max_iou: trim_mode 0 (joint / rcnn) or 1 (rpn), got %d", trim_mode);
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(boxes0 && (S == 1 || boxes1) && gt_boxes3d && gt_max && num_gt, "prcnn_eval_gt_max_iou: null pointer");
    EsGtMaxParams P;
    P.boxes0 = boxes0; P.boxes1 = boxes1; P.gt = gt_boxes3d; P.S = S; P.B = B; P.M = M; P.G = G; P.gt_cols = gt_cols; P.trim_mode = trim_mode;
    P.gt_max = gt_max; P.num_gt = num_gt;
    hipLaunchKernelGGL(es_gt_max_kernel, dim3(G, B, S), dim3(64), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_eval_gt_max_iou");
    return PRCNN_OK;
}

// LDS slots of the accumulate kernel
enum { ES_L_FRAME = 0,        // 6 x int: the current frame's correct / fg / pos, match-and-valid / valid / refined match
       ES_L_WORDS = 6 };

__global__ __launch_bounds__(ES_ACC_THREADS) void es_accumulate_kernel(const EsBatch P, EsState* st) {
    __shared__ unsigned long long s_cnt[12];             // recall 0..9, live ground truth, detections
    __shared__ unsigned long long s_all[3];              // the batch's correct / fg / pos (seg_mode 1)
    __shared__ int s_frame[ES_L_WORDS];
    const int tid = threadIdx.x;
    if (tid < 12) s_cnt[tid] = 0;
    if (tid < 3) s_all[tid] = 0;
    if (tid < ES_L_WORDS) s_frame[tid] = 0;
    __syncthreads();
    // recall: integer counts, any order
    if (P.G > 0) {
        for (int s = 0; s < P.S; s++) {
            unsigned c[ES_THRESHOLDS] = {0, 0, 0, 0, 0};
            for (long e = tid; e < (long)P.B * P.G; e += ES_ACC_THREADS) {
                const int b = (int)(e / P.G), j = (int)(e - (long)b * P.G);
                if (j >= P.num_gt[b]) continue;
                const float v = P.gt_max[(size_t)s * P.B * P.G + e];
                for (int t = 0; t < ES_THRESHOLDS; t++) c[t] += es_recalled(v, t) ? 1u : 0u;
            }
            for (int t = 0; t < ES_THRESHOLDS; t++)
                if (c[t]) atomicAdd(&s_cnt[(s ? ES_RECALL1 : ES_RECALL0) + t], (unsigned long long)c[t]);
        }
        for (int b = tid; b < P.B; b += ES_ACC_THREADS) atomicAdd(&s_cnt[ES_GT], (unsigned long long)P.num_gt[b]);
    }
    if (P.det_num)
        for (int b = tid; b < P.B; b += ES_ACC_THREADS) atomicAdd(&s_cnt[ES_DET], (unsigned long long)(long long)P.det_num[b]);
    // the ratios, frame by frame: counts through LDS, thread 0 divides, widens and adds -- the order of the reference's Python `+=`
    double seg_sum = 0.0, acc_sum = 0.0, ref_sum = 0.0;
    if (tid == 0) { seg_sum = st->sums[ES_SUM_SEG_IOU]; acc_sum = st->sums[ES_SUM_CLS_ACC]; ref_sum = st->sums[ES_SUM_CLS_ACC_REFINED]; }
    if (P.seg || P.pred_class) {
        for (int b = 0; b < P.B; b++) {
            int c[ES_L_WORDS] = {0, 0, 0, 0, 0, 0};
            if (P.seg)
                for (int64_t i = tid; i < P.N; i += ES_ACC_THREADS) {
                    const int bits = es_seg_point(P.seg[b * P.N + i], es_label_at(P.cls_label, P.label_is_i64, b * P.N + i));
                    c[0] += bits & 1; c[1] += (bits >> 1) & 1; c[2] += (bits >> 2) & 1;
                }
            if (P.pred_class)
                for (int r = tid; r < P.R; r += ES_ACC_THREADS) {
                    const int bits = es_cls_roi(P.pred_class[(size_t)b * P.R + r], P.gt_iou[(size_t)b * P.R + r], P.cls_fg, P.cls_bg, P.refine_thresh);
                    c[3] += bits & 1; c[4] += (bits >> 1) & 1; c[5] += (bits >> 2) & 1;
                }
            for (int q = 0; q < ES_L_WORDS; q++)
                if (c[q]) atomicAdd(&s_frame[q], c[q]);
            __syncthreads();
            if (tid == 0) {
                if (P.seg) {
                    if (P.seg_mode == 0) seg_sum += (double)es_seg_iou(s_frame[0], s_frame[1], s_frame[2]);
                    else for (int q = 0; q < 3; q++) s_all[q] += (unsigned long long)s_frame[q];
                }
                if (P.pred_class) {
                    acc_sum += (double)es_ratio(s_frame[3], s_frame[4]);
                    ref_sum += (double)es_ratio(s_frame[5], P.R);
                }
                for (int q = 0; q < ES_L_WORDS; q++) s_frame[q] = 0;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (P.seg && P.seg_mode == 1) {                  // eval_rcnn.py:568-573 inside `for k in range(batch_size)`: the batch's ratio, B times
            const double r = (double)es_seg_iou((int64_t)s_all[0], (int64_t)s_all[1], (int64_t)s_all[2]);
            for (int b = 0; b < P.B; b++) seg_sum += r;
        }
        for (int q = 0; q < 12; q++) st->counters[q] += (int64_t)s_cnt[q];
        st->counters[ES_FRAMES] += P.B;
        st->counters[ES_BATCHES] += 1;
        st->sums[ES_SUM_SEG_IOU] = seg_sum;
        st->sums[ES_SUM_CLS_ACC] = acc_sum;
        st->sums[ES_SUM_CLS_ACC_REFINED] = ref_sum;
    }
}

PRCNN_API int prcnn_eval_stats_accumulate(const float* gt_max, const int32_t* num_gt, int S, int B, int G, const int32_t* det_num,
                                          const float* seg, const void* cls_label, int label_is_i64, int64_t N, int seg_mode,
                                          const uint8_t* pred_class, const float* gt_iou, int R, float cls_fg, float cls_bg,
                                          float refine_thresh, void* state, prcnn_stream_t stream) {
    PRCNN_REQUIRE(S >= 0 && S <= 2 && B >= 1 && G >= 0 && G <= ES_MAX_GT, "prcnn_eval_stats_accumulate: bad shape S=%d (0..2) B=%d (>= 1) G=%d (0..%d)",
                  S, B, G, ES_MAX_GT);
    PRCNN_REQUIRE(state, "prcnn_eval_stats_accumulate: null state");
    PRCNN_REQUIRE(((uintptr_t)state & 7) == 0, "prcnn_eval_stats_accumulate: state must be 8-byte aligned");
    PRCNN_REQUIRE(S == 0 || G == 0 || (gt_max && num_gt), "prcnn_eval_stats_accumulate: gt_max / num_gt are null with S=%d G=%d", S, G);
    PRCNN_REQUIRE((seg != nullptr) == (cls_label != nullptr), "prcnn_eval_stats_accumulate: seg and cls_label come together (seg %s, cls_label %s)",
                  seg ? "given" : "null", cls_label ? "given" : "null");
    PRCNN_REQUIRE(!seg || (N >= 1 && N * (int64_t)B < ((int64_t)1 << 31) && (seg_mode == 0 || seg_mode == 1)),
                  "prcnn_eval_stats_accumulate: segmentation needs N >= 1, B * N < 2^31 and seg_mode 0 | 1 (N=%lld seg_mode=%d)", (long long)N, seg_mode);
    PRCNN_REQUIRE((pred_class != nullptr) == (gt_iou != nullptr), "prcnn_eval_stats_accumulate: pred_class and gt_iou come together");
    PRCNN_REQUIRE(!pred_class || R >= 1, "prcnn_eval_stats_accumulate: classification accuracy needs R >= 1 (got %d)", R);
    EsBatch P;
    P.gt_max = gt_max; P.num_gt = num_gt; P.S = (G > 0) ? S : 0; P.B = B; P.G = (S > 0) ? G : 0; P.det_num = det_num;
    P.seg = seg; P.cls_label = cls_label; P.label_is_i64 = label_is_i64; P.seg_mode = seg_mode; P.N = N;
    P.pred_class = pred_class; P.gt_iou = gt_iou; P.R = R; P.cls_fg = cls_fg; P.cls_bg = cls_bg; P.refine_thresh = refine_thresh;
    hipLaunchKernelGGL(es_accumulate_kernel, dim3(1), dim3(ES_ACC_THREADS), 0, (hipStream_t)stream, P, static_cast<EsState*>(state));
    PRCNN_LAUNCH_CHECK("prcnn_eval_stats_accumulate");
    return PRCNN_OK;
}
