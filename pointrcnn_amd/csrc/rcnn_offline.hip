// rcnn_offline.hip -- RoI sampling for RCNN offline training on the device (`train_rcnn.py --train_mode rcnn_offline`,
// RCNN.ROI_SAMPLE_JIT False): the sampling part of KittiRCNNDataset.get_rcnn_training_sample_batch
// (lib/datasets/kitti_rcnn_dataset.py:890-957) with sample_bg_inds (:1024-1050), aug_roi_by_noise_batch (:1052-1077) and
// random_aug_box3d (:747-788).  The reference runs it per frame on a dataloader worker, one shapely clip per box pair and one per
// noise attempt.  Here a batch is two launches and nothing returns to the host.
//
//   ro_iou_kernel     the (M x G) matrix of every frame spread over the chip, one lane per pair: get_iou3d on the float32 corners
//                     of both boxes (rcnn_offline_math.h; a separating axis decides most pairs without the clip)
//   ro_sample_kernel  one workgroup per frame:
//     1  row maximum and its label for every RoI (one lane per RoI, numpy's first maximum); column maximum and its RoI for every
//        label (one wave per label, lanes over the RoIs, combined to the first maximum)
//     2  (roi_sample.h, shared with the online sampler) the candidate lists in RoI order: foreground (row maximum >= min(REG_FG, CLS_FG)) FOLLOWED BY the best RoI of every label
//        whose column maximum is > 0, in label order -- an RoI can stand in that list several times (:894-901); hard and easy
//        background; the reference's cases; the picks
//     3  one lane per output slot: the noise loop (ten attempts on a foreground slot, one on a background slot, whose IoU is
//        recomputed too: iou_of_rois is always the loop's last IoU, never the matrix entry)
//
// Differences from the online sampler (proposal_target.hip): the IoU is the corner clip in double, not boxes_iou3d_gpu; the ground
// truth is counted (num_gt), not padded with zero rows; the foreground list holds the labels' best RoIs; the noisy box is float64;
// a frame with foreground but no background candidate makes the reference raise (:923, type_as on a numpy array) and is reported
// through status with its sampled outputs cleared.  Everything else of phase 2 -- lists, slot plan, ranks, picks, the decoding of cfg6,
// the noise range rows -- is roi_sample.h, one statement for both.
//
// Randomness (counter_rand.h; scene.hip's header lists every stream id), r(stream, frame, position):
//   stream 40, position = place t in the foreground list   np.random.permutation (:913): the slots go to the places with the
//                                                          smallest (key, t), in that order
//   stream 42 / 43, position = hard / easy slot            np.floor(np.random.rand(n) * len) (:1030-1045): below(r, len)
//   stream 50, position ((slot * 16 + attempt) * 16 + q)   the noise loop, see rcnn_offline_math.h
// (41 stays free: it would be the foreground draw with replacement of the case the reference raises on.)
// No atomics: the result depends on (seed, frame id, inputs) only.  frame_ids (B) gives the id that keys the table, so a batch
// packed in another order returns the same frames; NULL = the position in the batch.
#include "common.h"
#include "rcnn_offline_math.h"

constexpr int RO_THREADS = 256;
constexpr int RO_MAX_GT = 128;
constexpr int RO_MAX_ROI = 4096;
constexpr int RO_MAX_SLOTS = 1024;

struct RoParams {
    const float* roi;            // (B, M, 7)
    const int32_t* num_roi;      // (B)
    const float* gt;             // (B, G, 7)
    const int32_t* num_gt;       // (B)
    const int32_t* frame_ids;    // (B) or NULL
    int B, M, G, R;
    RsCfg c;
    int aug_times, aug_method;
    unsigned seed;
    float* iou;                  // (B, M, G)
    float* rois; float* gt_of_rois; float* roi_iou; int32_t* src;      // (B,R,7) (B,R,7) (B,R) (B,R)
    float* max_overlaps; int32_t* gt_assignment;                      // (B,M)
    int32_t* counts; int32_t* status;                                 // (B,4) (B)
};

__device__ __forceinline__ int ro_count(const int32_t* n, int b, int cap) { return min(max(n[b], 0), cap); }

__global__ __launch_bounds__(RO_THREADS) void ro_iou_kernel(const RoParams P) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * RO_THREADS + threadIdx.x;
    if (p >= P.M * P.G) return;
    const int i = p / P.G, j = p - i * P.G;
    float v = 0.0f;
    const int nr = ro_count(P.num_roi, b, P.M), ng = ro_count(P.num_gt, b, P.G);
    if (i < nr && j < ng) {
        float ca[24], cb[24];
        ro_corners_f32(P.roi + ((size_t)b * P.M + i) * 7, ca, nr == 1);       // a frame's only box: the one-box form (rcnn_offline_math.h)
        ro_corners_f32(P.gt + ((size_t)b * P.G + j) * 7, cb, ng == 1);
        v = ro_pair_iou(ca, cb);
    }
    P.iou[(size_t)b * P.M * P.G + p] = v;
}

__global__ __launch_bounds__(RO_THREADS) void ro_sample_kernel(const RoParams P) {
    extern __shared__ int lds_i[];                    // mo[M] (float), fg[M + G], hard[M], easy[M], keys[M + G]
    __shared__ int s_col[RO_MAX_GT];                  // the best RoI of every label, -1 when its column maximum is not > 0
    __shared__ RsLists s_lists;
    __shared__ RsPlan s_plan;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned frame = P.frame_ids ? (unsigned)P.frame_ids[b] : (unsigned)b;
    const float* roi = P.roi + (size_t)b * P.M * 7;
    const float* gt = P.gt + (size_t)b * P.G * 7;
    const float* iou = P.iou + (size_t)b * P.M * P.G;
    float* mo = reinterpret_cast<float*>(lds_i);
    int* fg = lds_i + P.M;
    int* hard = fg + P.M + P.G;
    int* easy = hard + P.M;
    unsigned* keys = reinterpret_cast<unsigned*>(easy + P.M);
    float* o_roi = P.rois + (size_t)b * P.R * 7;
    float* o_gt = P.gt_of_rois + (size_t)b * P.R * 7;
    float* o_iou = P.roi_iou + (size_t)b * P.R;
    int32_t* o_src = P.src + (size_t)b * P.R;
    const int nr = ro_count(P.num_roi, b, P.M), ng = ro_count(P.num_gt, b, P.G);

    rs_clear(o_roi, o_gt, o_iou, o_src, P.R, tid, RO_THREADS);
    // phase 1: iou3d.max(axis=1) / argmax(axis=1), rows past num_roi cleared
    for (int i = tid; i < P.M; i += RO_THREADS) {
        float best = 0.f;
        int arg = -1;
        if (i < nr && ng > 0) {
            best = iou[(size_t)i * P.G]; arg = 0;
            for (int j = 1; j < ng; j++) {
                const float v = iou[(size_t)i * P.G + j];
                if (v > best) { best = v; arg = j; }
            }
        }
        mo[i] = best;
        P.max_overlaps[(size_t)b * P.M + i] = best;
        P.gt_assignment[(size_t)b * P.M + i] = arg;
    }
    if (tid == 0) {
        // 2: max of an empty array (:893); 1: argmax over no RoI (:894)
        P.status[b] = ng == 0 ? 2 : (nr == 0 ? 1 : 0);
        for (int q = 0; q < 4; q++) P.counts[b * 4 + q] = 0;
    }
    if (ng == 0 || nr == 0) return;
    // iou3d.max(axis=0) / argmax(axis=0): a wave per label, the lanes' first maxima combined to the first maximum
    for (int j = wave; j < ng; j += RO_THREADS / 64) {
        float best = -INFINITY;
        int arg = 0x7fffffff;
        for (int i = lane; i < nr; i += 64) {
            const float v = iou[(size_t)i * P.G + j];
            if (v > best) { best = v; arg = i; }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(arg, o);
            if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (lane == 0) s_col[j] = best > 0.f ? arg : -1;
    }
    for (int t = tid; t < P.M + P.G; t += RO_THREADS) keys[t] = scene_rand(P.seed, RO_STREAM_FG_KEY, frame, (unsigned)t);
    __syncthreads();
    // phase 2: the lists in RoI order, then the reference's cases.  One lane walks mo[] in LDS while 255 wait: M dependent LDS reads,
    // by the LDS latency an estimated 1 - 2 us at the workload's M = 300 and 20 - 30 us at the cap of 4096 (not timed on its own; the
    // whole call measures 181 us at M = 300 and 643 us at the cap).  A prefix scan would buy back that part only.
    if (tid == 0) {
        RsLists l = rs_lists(mo, nr, P.c, fg, hard, easy);
        for (int j = 0; j < ng; j++)
            if (s_col[j] >= 0) fg[l.nfg++] = s_col[j];
        const RsPlan p = rs_plan(l, P.R, P.c.fg_per_image, P.c.hard_ratio);
        if (p.kind == RS_FG_ONLY || p.kind == RS_NEITHER) P.status[b] = 1;      // foreground only (:923 raises), or no candidate at all (:932-935)
        s_lists = l; s_plan = p;
        P.counts[b * 4] = l.nfg; P.counts[b * 4 + 1] = l.nhard; P.counts[b * 4 + 2] = l.neasy; P.counts[b * 4 + 3] = p.fs;
    }
    __syncthreads();
    const RsLists l = s_lists;
    const RsPlan p = s_plan;
    const int fs = p.fs;
    if (fs + p.bs == 0) return;
    for (int t = tid; t < l.nfg && fs > 0; t += RO_THREADS) {
        const int rank = rs_rank(keys, l.nfg, t);
        if (rank < fs) o_src[rank] = fg[t];
    }
    for (int t = tid; t < p.bs; t += RO_THREADS)
        o_src[fs + t] = rs_bg_pick(t, p, l, hard, easy, P.seed, RO_STREAM_HARD, RO_STREAM_EASY, frame);
    __syncthreads();
    // phase 3: aug_roi_by_noise_batch
    for (int t = tid; t < P.R; t += RO_THREADS) {
        const int i = o_src[t];
        const int ga = P.gt_assignment[(size_t)b * P.M + i];
        float box[7], g[7], gc[24], out[7], v;
        for (int c = 0; c < 7; c++) { box[c] = roi[(size_t)i * 7 + c]; g[c] = gt[(size_t)ga * 7 + c]; }
        ro_corners_f32(g, gc, true);
        ro_noise_slot(box, gc, t < fs ? P.aug_times : min(P.aug_times, 1), P.c.pos_thresh, P.seed, frame, (unsigned)t, P.aug_method, out, &v);
        for (int c = 0; c < 7; c++) { o_roi[(size_t)t * 7 + c] = out[c]; o_gt[(size_t)t * 7 + c] = g[c]; }
        o_iou[t] = v;
    }
}

PRCNN_API int prcnn_rcnn_offline_sample(const float* roi_boxes3d, const int32_t* num_roi, const float* gt_boxes3d, const int32_t* num_gt,
                                        const int32_t* frame_ids, int B, int M, int G, int roi_per_image, const double* cfg6, int aug_times,
                                        int aug_method, uint32_t seed, float* iou3d, float* rois, float* gt_of_rois, float* roi_iou,
                                        int32_t* src, float* max_overlaps, int32_t* gt_assignment, int32_t* counts, int32_t* status,
                                        prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && M > 0 && M <= RO_MAX_ROI && G > 0 && G <= RO_MAX_GT && roi_per_image > 0 && roi_per_image <= RO_MAX_SLOTS,
                  "prcnn_rcnn_offline_sample: bad shape B=%d M=%d (<= %d) G=%d (<= %d) R=%d (<= %d)", B, M, RO_MAX_ROI, G, RO_MAX_GT,
                  roi_per_image, RO_MAX_SLOTS);
    PRCNN_REQUIRE(aug_times >= 0 && aug_times <= RO_MAX_AUG_TIMES && (aug_method == 0 || aug_method == 1),
                  "prcnn_rcnn_offline_sample: aug_times in 0..16, aug_method 0 ('multiple') or 1 ('single')");
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(roi_boxes3d && num_roi && gt_boxes3d && num_gt && cfg6 && iou3d && rois && gt_of_rois && roi_iou && src && max_overlaps &&
                  gt_assignment && counts && status, "prcnn_rcnn_offline_sample: null pointer");
    RoParams P;
    P.roi = roi_boxes3d; P.num_roi = num_roi; P.gt = gt_boxes3d; P.num_gt = num_gt; P.frame_ids = frame_ids;
    P.B = B; P.M = M; P.G = G; P.R = roi_per_image;
    P.c = rs_cfg(cfg6, roi_per_image);
    P.aug_times = aug_times; P.aug_method = aug_method; P.seed = seed;
    P.iou = iou3d; P.rois = rois; P.gt_of_rois = gt_of_rois; P.roi_iou = roi_iou; P.src = src; P.max_overlaps = max_overlaps;
    P.gt_assignment = gt_assignment; P.counts = counts; P.status = status;
    hipLaunchKernelGGL(ro_iou_kernel, dim3(prcnn_divup((long)M * G, RO_THREADS), B), dim3(RO_THREADS), 0, (hipStream_t)stream, P);
    // mo / fg / hard / easy / keys: (5 M + 2 G) words of dynamic LDS, 81 KB at the caps
    const size_t lds = ((size_t)M * 5 + (size_t)G * 2) * sizeof(int);
    static PrcnnLdsLimit attr;
    PRCNN_REQUIRE(lds <= 48 * 1024 || attr.raise((const void*)ro_sample_kernel, (RO_MAX_ROI * 5 + RO_MAX_GT * 2) * (int)sizeof(int)),
                  "prcnn_rcnn_offline_sample: cannot raise the dynamic LDS limit for M=%d", M);
    hipLaunchKernelGGL(ro_sample_kernel, dim3(B), dim3(RO_THREADS), lds, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_rcnn_offline_sample");
    return PRCNN_OK;
}

// ------------------------------------------------------------------------------------------------ after pooling
// prcnn_rcnn_offline_finish: everything of get_rcnn_training_sample_batch after roipool3d_cpu (:976-1010) in one pass over the pooled
// (B * R, S, ld) tensor, touching its xyz columns only.  One workgroup per slot: every lane forms the slot's augmentation and
// canonical frame (a few dozen operations, cheaper than a broadcast), lane 0 writes the slot's boxes and labels, the lanes walk the
// S points.  A frame whose status is not 0 has no sampled RoI: its pooled rows (all columns) and boxes are cleared, label -1, mask 0.
struct RoFinishParams {
    float* pooled; int ld;       // (B * R, S, ld), xyz in columns 0:3, rewritten in place
    int B, R, S;
    const float* rois; const float* gt_of_rois; const float* roi_iou;      // (B,R,7) (B,R,7) (B,R): the sampler's
    const int32_t* empty;        // (B, R) pooled_empty_flag
    const int32_t* status;       // (B) the sampler's
    const int32_t* frame_ids;    // (B) or NULL
    int methods;
    double flip_prob, rot_range;
    float reg_fg, cls_fg, cls_bg;
    unsigned seed;
    float* out_rois; float* out_gt; float* out_ct;      // (B,R,7) each
    int32_t* cls_label; int32_t* reg_valid_mask;        // (B,R)
};

__global__ __launch_bounds__(RO_THREADS) void ro_finish_kernel(const RoFinishParams P) {
    const int row = blockIdx.x, b = row / P.R, t = row - b * P.R, tid = threadIdx.x;
    float* pts = P.pooled + (size_t)row * P.S * P.ld;
    if (P.status[b] != 0) {
        for (int e = tid; e < P.S * P.ld; e += RO_THREADS) pts[e] = 0.f;      // every column: what was pooled there belongs to no RoI
        if (tid == 0) {
            for (int c = 0; c < 7; c++) { P.out_rois[(size_t)row * 7 + c] = 0.f; P.out_gt[(size_t)row * 7 + c] = 0.f; P.out_ct[(size_t)row * 7 + c] = 0.f; }
            P.cls_label[row] = -1; P.reg_valid_mask[row] = 0;
        }
        return;
    }
    const unsigned frame = P.frame_ids ? (unsigned)P.frame_ids[b] : (unsigned)b;
    const RoAug a = ro_aug_draw(P.seed, frame, (unsigned)t, P.methods, P.flip_prob, P.rot_range);
    float roi[7], gt[7], ct[7];
    for (int c = 0; c < 7; c++) { roi[c] = P.rois[(size_t)row * 7 + c]; gt[c] = P.gt_of_rois[(size_t)row * 7 + c]; }
    const RoCanon cn = ro_finish_boxes(roi, gt, a, ct);
    if (tid == 0) {
        for (int c = 0; c < 7; c++) { P.out_rois[(size_t)row * 7 + c] = roi[c]; P.out_gt[(size_t)row * 7 + c] = gt[c]; P.out_ct[(size_t)row * 7 + c] = ct[c]; }
        int mask;
        P.cls_label[row] = ro_labels(P.roi_iou[row], P.empty[row], P.reg_fg, P.cls_fg, P.cls_bg, &mask);
        P.reg_valid_mask[row] = mask;
    }
    for (int s = tid; s < P.S; s += RO_THREADS) {
        float p[3] = {pts[(size_t)s * P.ld], pts[(size_t)s * P.ld + 1], pts[(size_t)s * P.ld + 2]};
        ro_aug_point(p, a);
        ro_canon_point(p, cn);
        pts[(size_t)s * P.ld] = p[0]; pts[(size_t)s * P.ld + 1] = p[1]; pts[(size_t)s * P.ld + 2] = p[2];
    }
}

PRCNN_API int prcnn_rcnn_offline_finish(float* pooled, int ld, int B, int R, int S, const float* rois, const float* gt_of_rois,
                                        const float* roi_iou, const int32_t* pooled_empty_flag, const int32_t* status,
                                        const int32_t* frame_ids, const double* cfg5, int aug_methods, uint32_t seed, float* out_rois,
                                        float* out_gt_of_rois, float* gt_boxes3d_ct, int32_t* cls_label, int32_t* reg_valid_mask,
                                        prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && R > 0 && S > 0 && ld >= 3 && (long)B * R <= 0x7fffffffL, "prcnn_rcnn_offline_finish: bad shape B=%d R=%d S=%d ld=%d", B, R, S, ld);
    PRCNN_REQUIRE(aug_methods >= 0 && aug_methods <= 7, "prcnn_rcnn_offline_finish: aug_methods is a mask of rotation 1, scaling 2, flip 4");
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(pooled && rois && gt_of_rois && roi_iou && pooled_empty_flag && status && cfg5 && out_rois && out_gt_of_rois &&
                  gt_boxes3d_ct && cls_label && reg_valid_mask, "prcnn_rcnn_offline_finish: null pointer");
    PRCNN_REQUIRE(!(aug_methods & 1) || cfg5[4] > 0.0, "prcnn_rcnn_offline_finish: AUG_ROT_RANGE must be positive");
    RoFinishParams P;
    P.pooled = pooled; P.ld = ld; P.B = B; P.R = R; P.S = S; P.rois = rois; P.gt_of_rois = gt_of_rois; P.roi_iou = roi_iou;
    P.empty = pooled_empty_flag; P.status = status; P.frame_ids = frame_ids; P.methods = aug_methods;
    P.reg_fg = (float)cfg5[0]; P.cls_fg = (float)cfg5[1]; P.cls_bg = (float)cfg5[2]; P.flip_prob = cfg5[3]; P.rot_range = cfg5[4];
    P.seed = seed; P.out_rois = out_rois; P.out_gt = out_gt_of_rois; P.out_ct = gt_boxes3d_ct; P.cls_label = cls_label;
    P.reg_valid_mask = reg_valid_mask;
    hipLaunchKernelGGL(ro_finish_kernel, dim3(B * R), dim3(RO_THREADS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_rcnn_offline_finish");
    return PRCNN_OK;
}
