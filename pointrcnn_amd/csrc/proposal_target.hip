// proposal_target.hip -- RCNN-stage training targets on the device: RoI sampling + noise augmentation.
//
// Replaces ProposalTargetLayer.sample_rois_for_rcnn / sample_bg_inds / aug_roi_by_noise_torch / random_aug_box3d
// (lib/rpn/proposal_target_layer.py:75-300) and the iou3d_utils.boxes_iou3d_gpu calls inside them
// (lib/utils/iou3d/iou3d_utils.py:20-53).  The reference walks the batch in a Python loop; per frame it launches one
// (M x G) overlap kernel, about thirty small torch kernels with four host synchronisations (torch.nonzero, .numel()), and then,
// for each of the 64 sampled RoIs, a Python `while` loop of up to ten attempts that each build a box on the device, launch a
// 1 x 1 overlap kernel and read the IoU back (`temp_iou < pos_thresh` on the host): ~700 blocking round trips per frame.
// Here a frame is one workgroup and one launch covers the batch; nothing returns to the host.
//
//   phase 1  thread per RoI: 3-D IoU against every ground-truth box (rotated BEV overlap of iou3d_geom.h x height overlap /
//            union volume, each operation individually rounded as the torch expression does), first maximum + its index
//   phase 2  the three candidate lists (foreground >= min(REG_FG, CLS_FG); hard background in [BG_LO, BG); easy < BG_LO) in RoI
//            order, the reference's four cases, the picks
//   phase 3  thread per output slot: the accept / retry loop of aug_roi_by_noise_torch with random_aug_box3d inline
//
// Randomness is re-specified (the reference draws from numpy's and torch's global streams in a data-dependent order) with the
// counter-based generator of scene.hip, one number per (purpose, frame, position):
//   stream 10, index = RoI            fg keys: sampling without replacement = the RoIs with the smallest (key, RoI), in that order
//                                     (the list is in RoI order, so (key, RoI) orders it as roi_sample.h's (key, place) does)
//   stream 11, index = slot           fg sampling with replacement (frames without a background candidate)
//   stream 12 / 13, index = position  hard / easy background picks
//   stream 20, index = ((slot * 16 + attempt) * 16 + q): q = 8 keep-the-original decision (u < 0.2), q = 0 range row,
//                                     q = 1..3 position shift, q = 4..6 size scale, q = 7 rotation
// tests/golden/ref_proposal_target.py answers the reference's own random calls from the same table: its output must be -- and is
// -- reproduced bit for bit by the oracle in reference arithmetic; this kernel equals the oracle in the kernels' arithmetic
// (box trigonometry in double rounded once, division-only vertex order: DESIGN.md section 2).
#include "iou3d_pair.h"
#include "roi_sample.h"

#define PT_THREADS 256
#define PT_MAX_GT 128
constexpr unsigned PT_STREAM_FG_KEY = 10, PT_STREAM_FG_REPLACE = 11, PT_STREAM_HARD = 12, PT_STREAM_EASY = 13, PT_STREAM_NOISE = 20;

// bev_of, iou3d_pair, live_gt: iou3d_pair.h (shared with eval_stats.hip); the selection of phase 2: roi_sample.h (shared with rcnn_offline.hip)

struct PtParams {
    const float* roi;        // (B, M, 7)
    const float* gt;         // (B, G, gt_cols)
    int B, M, G, gt_cols, R;
    RsCfg c;
    int aug_times, aug_method;
    unsigned seed;
    float* rois; float* gt_of_rois; float* roi_iou; int32_t* src;      // (B,R,7) (B,R,7) (B,R) (B,R)
    float* max_overlaps; int32_t* gt_assignment;                      // (B,M)
    int32_t* counts; int32_t* status;                                 // (B,4) (B)
};

// Phase 1 on the whole chip: max IoU and its ground-truth box for every RoI (iou3d_utils.boxes_iou3d_gpu + torch.max over dim 1,
// :100-101).  The sampler kernel below is one workgroup per frame -- its branching is per frame -- and 512 RoIs x 12 boxes of
// rotated-polygon clipping on one workgroup was 400 of its 650 us.  Here a wave takes 4 RoIs, 16 lanes per RoI over the ground truth;
// lanes combine to the FIRST maximum (torch.max's rule: ties -> lowest index; a NaN only counts in column 0, as in the sequential
// `j == 0 || v > best` scan of the sampler's own reference).
__global__ __launch_bounds__(64) void pt_overlaps_kernel(const PtParams P) {
    const int b = blockIdx.y, lane = threadIdx.x;
    const int i = blockIdx.x * 4 + (lane >> 4), sub = lane & 15;
    const float* gt = P.gt + (size_t)b * P.G * P.gt_cols;
    const int ng = live_gt(gt, P.G, P.gt_cols, 0);
    const bool live = i < P.M;
    if (ng == 0) {                                      // status 2: every output byte is defined, 0 / 0 as the oracle reports it
        if (live && sub == 0) { P.max_overlaps[(size_t)b * P.M + i] = 0.f; P.gt_assignment[(size_t)b * P.M + i] = 0; }
        return;
    }
    float a[7];
    for (int c = 0; c < 7; c++) a[c] = P.roi[((size_t)b * P.M + (live ? i : 0)) * 7 + c];
    float best = -INFINITY, v0 = 0.f;
    int arg = 0x7fffffff;
    for (int j = sub; j < ng; j += 16) {
        float g[7], bev[5];
        RBox rb;
        for (int c = 0; c < 7; c++) g[c] = gt[(size_t)j * P.gt_cols + c];
        bev_of(g, bev);
        make_rbox(bev, rb);
        const float v = iou3d_pair(a, g, rb);
        if (j == 0) v0 = v;
        if (v > best || (v == best && j < arg)) { best = v; arg = j; }
    }
    for (int o = 8; o > 0; o >>= 1) {                   // within the RoI's 16 lanes
        const float ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    v0 = __shfl(v0, lane & ~15);
    if (v0 != v0 || arg == 0x7fffffff) { best = v0; arg = 0; }      // NaN in column 0 / nothing but NaNs: what the sequential scan keeps
    if (live && sub == 0) {
        P.max_overlaps[(size_t)b * P.M + i] = best;
        P.gt_assignment[(size_t)b * P.M + i] = arg;
    }
}

__global__ __launch_bounds__(PT_THREADS) void proposal_target_kernel(const PtParams P) {
    extern __shared__ int lds_i[];                    // fg[M], hard[M], easy[M] candidate lists, then keys[M]
    __shared__ RBox s_gt[PT_MAX_GT];
    __shared__ float s_gtraw[PT_MAX_GT][7];
    __shared__ int s_ng;
    __shared__ RsLists s_lists;
    __shared__ RsPlan s_plan;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* roi = P.roi + (size_t)b * P.M * 7;
    const float* gt = P.gt + (size_t)b * P.G * P.gt_cols;
    int* fg = lds_i;
    int* hard = fg + P.M;
    int* easy = hard + P.M;
    unsigned* keys = reinterpret_cast<unsigned*>(easy + P.M);
    float* o_roi = P.rois + (size_t)b * P.R * 7;
    float* o_gt = P.gt_of_rois + (size_t)b * P.R * 7;
    float* o_iou = P.roi_iou + (size_t)b * P.R;
    int32_t* o_src = P.src + (size_t)b * P.R;
    const float fg_thresh = P.c.fg_thresh;

    if (tid == 0) {                                   // :96-99: drop the all-zero rows at the end of the ground truth
        const int ng = live_gt(gt, P.G, P.gt_cols, 0);
        s_ng = ng;
        P.status[b] = ng == 0 ? 2 : 0;
        for (int q = 0; q < 4; q++) P.counts[b * 4 + q] = 0;
    }
    rs_clear(o_roi, o_gt, o_iou, o_src, P.R, tid, PT_THREADS);
    __syncthreads();
    const int ng = s_ng;
    if (ng == 0) return;
    for (int j = tid; j < ng; j += PT_THREADS) {
        float bev[5];
        for (int c = 0; c < 7; c++) s_gtraw[j][c] = gt[(size_t)j * P.gt_cols + c];
        bev_of(s_gtraw[j], bev);
        make_rbox(bev, s_gt[j]);
    }
    // phase 1 (max_overlaps / gt_assignment): pt_overlaps_kernel, launched before this one
    // phase 2: candidate lists in RoI order (one thread: M <= a few thousand), then the reference's four cases (roi_sample.h)
    if (tid == 0) {
        const RsLists l = rs_lists(P.max_overlaps + (size_t)b * P.M, P.M, P.c, fg, hard, easy);
        RsPlan p = rs_plan(l, P.R, P.c.fg_per_image, P.c.hard_ratio);
        if (p.kind == RS_FG_ONLY) p.fs = P.R;         // no background candidate: every slot is foreground, with replacement (:137-141)
        if (p.kind == RS_NEITHER) P.status[b] = 1;
        s_lists = l; s_plan = p;
        P.counts[b * 4] = l.nfg; P.counts[b * 4 + 1] = l.nhard; P.counts[b * 4 + 2] = l.neasy; P.counts[b * 4 + 3] = p.fs;
    }
    __syncthreads();
    const RsLists l = s_lists;
    const RsPlan p = s_plan;
    const int fs = p.fs;
    if (p.kind == RS_NEITHER) return;
    if (p.kind == RS_BOTH) {
        for (int t = tid; t < l.nfg; t += PT_THREADS) keys[t] = scene_rand(P.seed, PT_STREAM_FG_KEY, (unsigned)b, (unsigned)fg[t]);
        __syncthreads();                              // p.kind is the workgroup's: every lane is here
        for (int t = tid; t < l.nfg; t += PT_THREADS) {
            const int rank = rs_rank(keys, l.nfg, t);
            if (rank < fs) o_src[rank] = fg[t];
        }
    } else if (p.kind == RS_FG_ONLY) {
        for (int t = tid; t < P.R; t += PT_THREADS)
            o_src[t] = fg[rs_below(scene_rand(P.seed, PT_STREAM_FG_REPLACE, (unsigned)b, (unsigned)t), l.nfg)];
    }
    for (int t = tid; t < p.bs; t += PT_THREADS)
        o_src[fs + t] = rs_bg_pick(t, p, l, hard, easy, P.seed, PT_STREAM_HARD, PT_STREAM_EASY, (unsigned)b);
    __syncthreads();
    // phase 3: aug_roi_by_noise_torch
    for (int t = tid; t < P.R; t += PT_THREADS) {
        const int i = o_src[t];
        const int ga = P.gt_assignment[(size_t)b * P.M + i];
        const float iou_src = P.max_overlaps[(size_t)b * P.M + i];
        float box[7], aug[7];
        for (int c = 0; c < 7; c++) { box[c] = roi[(size_t)i * 7 + c]; aug[c] = box[c]; }
        const int times = t < fs ? P.aug_times : (P.aug_times > 0 ? 1 : 0);
        float temp_iou = 0.f;
        int cnt = 0;
        bool keep = true;
        while (temp_iou < fg_thresh && cnt < times) {
            const unsigned base = (unsigned)((t * 16 + cnt) * 16);
            if (scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 8)) < 0.2f) {
                for (int c = 0; c < 7; c++) aug[c] = box[c];
                keep = true;
            } else {
                float ps[3], hs[3], ar;
                if (P.aug_method == 0) {                     // 'multiple' (:262-277)
                    const RsNoiseRange rg = rs_noise_range(rs_below(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base), 5));
                    for (int c = 0; c < 3; c++) ps[c] = mul(sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 1 + c)), 0.5f) / 0.5f, (float)rg.pos);
                    for (int c = 0; c < 3; c++) hs[c] = add(mul(sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 4 + c)), 0.5f) / 0.5f, (float)rg.hwl), 1.0f);
                    ar = mul(sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 7)), 0.5f) / 0.5f, (float)rg.ang);
                } else {                                     // 'single' (:254-260)
                    for (int c = 0; c < 3; c++) ps[c] = sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 1 + c)), 0.5f);
                    for (int c = 0; c < 3; c++) hs[c] = add(sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 4 + c)), 0.5f) / (float)(0.5 / 0.15), 1.0f);
                    ar = sub(scene_u01f(scene_rand(P.seed, PT_STREAM_NOISE, (unsigned)b, base + 7)), 0.5f) / (float)(0.5 / (3.14159265358979323846 / 12));
                }
                for (int c = 0; c < 3; c++) { aug[c] = add(box[c], ps[c]); aug[3 + c] = mul(box[3 + c], hs[c]); }
                aug[6] = add(box[6], ar);
                keep = false;
            }
            temp_iou = iou3d_pair(aug, s_gtraw[ga], s_gt[ga]);
            cnt++;
        }
        for (int c = 0; c < 7; c++) { o_roi[(size_t)t * 7 + c] = aug[c]; o_gt[(size_t)t * 7 + c] = s_gtraw[ga][c]; }
        o_iou[t] = (cnt == 0 || keep) ? iou_src : temp_iou;
    }
}

PRCNN_API int prcnn_proposal_target_sample(const float* roi_boxes3d, const float* gt_boxes3d, int B, int M, int G, int gt_cols,
                                           int roi_per_image, const double* cfg6, int aug_times, int aug_method, uint32_t seed,
                                           float* rois, float* gt_of_rois, float* roi_iou, int32_t* src, float* max_overlaps,
                                           int32_t* gt_assignment, int32_t* counts, int32_t* status, prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && M > 0 && G > 0 && G <= PT_MAX_GT && gt_cols >= 7 && roi_per_image > 0,
                  "prcnn_proposal_target_sample: bad shape B=%d M=%d G=%d (<= %d) gt_cols=%d R=%d", B, M, G, PT_MAX_GT, gt_cols, roi_per_image);
    PRCNN_REQUIRE(M <= 8192, "prcnn_proposal_target_sample: at most 8192 RoIs per frame (got %d)", M);
    PRCNN_REQUIRE(aug_times >= 0 && aug_times <= 16 && (aug_method == 0 || aug_method == 1),
                  "prcnn_proposal_target_sample: aug_times in 0..16, aug_method 0 ('multiple') or 1 ('single')");
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(roi_boxes3d && gt_boxes3d && cfg6 && rois && gt_of_rois && roi_iou && src && max_overlaps && gt_assignment && counts && status,
                  "prcnn_proposal_target_sample: null pointer");
    PtParams P;
    P.roi = roi_boxes3d; P.gt = gt_boxes3d; P.B = B; P.M = M; P.G = G; P.gt_cols = gt_cols; P.R = roi_per_image;
    P.c = rs_cfg(cfg6, roi_per_image);
    P.aug_times = aug_times; P.aug_method = aug_method; P.seed = seed;
    P.rois = rois; P.gt_of_rois = gt_of_rois; P.roi_iou = roi_iou; P.src = src; P.max_overlaps = max_overlaps;
    P.gt_assignment = gt_assignment; P.counts = counts; P.status = status;
    hipLaunchKernelGGL(pt_overlaps_kernel, dim3(prcnn_divup(M, 4), B), dim3(64), 0, (hipStream_t)stream, P);
    // keys / fg / hard / easy lists: 16 bytes per RoI of dynamic LDS (128 KB at the 8192-RoI cap) next to ~12 KB static
    const size_t lds = (size_t)M * 4 * sizeof(int);
    static PrcnnLdsLimit attr;
    PRCNN_REQUIRE(lds <= 48 * 1024 || attr.raise((const void*)proposal_target_kernel, 8192 * 4 * (int)sizeof(int)),
                  "prcnn_proposal_target_sample: cannot raise the dynamic LDS limit for M=%d", M);
    hipLaunchKernelGGL(proposal_target_kernel, dim3(B), dim3(PT_THREADS), lds, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_proposal_target_sample");
    return PRCNN_OK;
}

// iou3d_utils.boxes_iou3d_gpu as one kernel: out (Na, Nb)
__global__ __launch_bounds__(256) void boxes_iou3d_kernel(const float* __restrict__ a, int Na, const float* __restrict__ b, int Nb,
                                                          float* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Na * Nb) return;
    const int i = (int)(e / Nb), j = (int)(e - (long)i * Nb);
    float bb[7], bev[5];
    for (int c = 0; c < 7; c++) bb[c] = b[(size_t)j * 7 + c];
    bev_of(bb, bev);
    RBox rb;
    make_rbox(bev, rb);
    float aa[7];
    for (int c = 0; c < 7; c++) aa[c] = a[(size_t)i * 7 + c];
    out[e] = iou3d_pair(aa, bb, rb);
}

PRCNN_API int prcnn_boxes_iou3d(const float* a, int Na, const float* b, int Nb, float* out, prcnn_stream_t stream) {
    PRCNN_REQUIRE(Na >= 0 && Nb >= 0, "prcnn_boxes_iou3d: bad shape");
    if (Na == 0 || Nb == 0) return PRCNN_OK;
    PRCNN_REQUIRE(a && b && out, "prcnn_boxes_iou3d: null pointer");
    hipLaunchKernelGGL(boxes_iou3d_kernel, dim3(prcnn_divup((long)Na * Nb, 256)), dim3(256), 0, (hipStream_t)stream, a, Na, b, Nb, out);
    PRCNN_LAUNCH_CHECK("prcnn_boxes_iou3d");
    return PRCNN_OK;
}
