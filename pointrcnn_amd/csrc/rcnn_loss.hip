// rcnn_loss.hip -- the RCNN training loss (train_functions.get_rcnn_loss: BinaryCrossEntropy or SigmoidFocalLoss classification +
// bin-based box regression with the fine angle target over the rows reg_valid_mask selects) and its gradient on the device
// (arithmetic: rcnn_loss_math.h).  The work is launch-bound (256 rows per training step), so the launches are few, not wide.
//
//   prcnn_rcnn_loss_forward   one launch over all rows (RC_ROWS rows per workgroup, one lane per row): the classification term of
//                             every row with label >= 0 and the nine regression terms of every row with mask > 0, UNNORMALISED, summed
//                             per workgroup in double in a fixed order.  The loss is linear in its normalisers, so the counts need no
//                             pass of their own: workgroup 0 also counts pos = #(label > 0), valid = #(label >= 0), fg = #(mask > 0)
//                             and the mask's sum over all rows as integers.  With finalize != 0 the single-process result follows: in
//                             the same launch when the grid is one workgroup, else in a second launch.
//   prcnn_rcnn_loss_finalize  one workgroup: sums the per-workgroup partials in a fixed order and applies the means (divisor count x
//                             columns; an empty selection gives 0), 3 x size, the normalisers and the total.  A data-parallel caller
//                             runs the forward with finalize = 0, all-reduces the counts and passes its scalings here.
//   prcnn_rcnn_loss_backward  one launch, the forward's geometry, grad_output read from the device: d loss / d rcnn_cls and
//                             d loss / d rcnn_reg, every entry written exactly once (zeros where no term is carried; no memset, no atomics).
// A regression row may have any channel count up to RC_MAX_C at any 4-byte-aligned address and stride (46 and 53 for the stock heads: no
// 8- or 16-byte unit fits), so rows are staged element by element, coalesced over the flat (row, channel) index, into LDS at an ODD row
// stride (C | 1: the lanes of a wave, one row each, then hit distinct banks), where the row's lane works on them in place.  A row whose
// mask is 0 is never read, nor its labels (reg_valid_mask is a 0 / 1 flag: the kernel selects by > 0, and the sum it reports next to the
// count is taken over the values' low 32 bits); a row with label -1 never has its logit read.  The grid is a function of the row count
// alone, and no result depends on anything but the rows in their flat order.
#include "common.h"
#include "rcnn_loss_math.h"

constexpr int RC_ROWS = 256;              // rows per workgroup = lanes per workgroup: a training step's 256 RoIs are one workgroup
constexpr int RC_MAX_C = 56;              // widest regression row held in LDS (46 / 53 for the stock heads); ops.RCNN_LOSS_MAX_C
constexpr int RC_LDC = RC_MAX_C | 1;
constexpr int RC_WAVES = RC_ROWS / 64;
constexpr int64_t RC_MAX_ROWS = (int64_t)1 << 24;      // the counts leave as float32 in the term vector; ops.RCNN_LOSS_MAX_ROWS

static inline int rc_blocks(int64_t npts) { return (int)((npts + RC_ROWS - 1) / RC_ROWS); }

__device__ __forceinline__ int64_t rc_int(const void* p, int is_i64, int64_t r) {
    return is_i64 ? ((const int64_t*)p)[r] : (int64_t)((const int32_t*)p)[r];
}
__device__ __forceinline__ int rc_sign(int64_t v) { return v > 0 ? 1 : (v == 0 ? 0 : -1); }

struct RcParams {
    const float* cls;           // row r's logit at cls[r * ld_cls]
    const float* reg;           // row r's C predictions at reg + r * ld_reg
    int64_t ld_cls, ld_reg;
    const void* label;          // (npts) i32 or i64: > 0 positive, 0 negative, < 0 ignored
    const void* mask;           // (npts) i32 or i64: > 0 the row is regressed
    int label_i64, mask_i64;
    const float* roi;           // (npts, 7): columns 3..5 are the per-row anchor
    const float* gt;            // (npts, 7) [dx dy dz h w l ry]
    int64_t npts;
    const float* norm;          // null (single process) or {classification scale, regression scale}
    int32_t* counts;            // forward: written {pos, valid, fg, mask sum}; backward: read
    const float* grad_out;      // backward: the upstream scalar
    float* dcls;                // backward: (npts)
    float* dreg;                // backward: (npts, C) contiguous
    double* partial;            // forward: (blocks, RC_TERMS)
    float* terms;               // forward with finalize: (23)
    int finalize;
    RcConfig cfg;
};

// t: the RC_TERMS unnormalised sums; counts {pos, valid, fg, mask sum}; norm null or {cls scale, reg scale} -> terms (23), doubles
// rounded to float once at the end
__device__ void rc_finalize(const double* t, const int32_t* counts, const float* norm, const RcConfig& cfg, float* terms) {
    const int n_cls = cfg.loss_cls == RC_LOSS_FOCAL ? counts[0] : counts[1];
    const int fg = counts[2];
    const double w = norm ? (double)norm[0] : 1.0 / (double)(n_cls > 1 ? n_cls : 1);
    const double scale = norm ? (double)norm[1] : 1.0;
    const double cnt = (double)(fg > 1 ? fg : 1);
    double head[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) head[k] = t[RC_X_BIN + k] / cnt;          // without LOC_Y_BY_BIN the y_res sum is 0
    const double size_mean = t[RC_SIZE] / (cnt * 3.0);
    const double loc = head[0] + head[1] + head[2] + head[3] + head[4] + head[5];
    const double angle = head[6] + head[7];
    const double loc_s = loc * scale, angle_s = angle * scale, size_s = 3.0 * size_mean * scale;
    const double reg = loc_s + angle_s + size_s;
    const double cls = t[RC_CLS] * w;
    terms[0] = (float)(cls + reg);
    terms[1] = (float)cls;
    terms[2] = (float)reg;
    terms[3] = (float)loc_s;
    terms[4] = (float)angle_s;
    terms[5] = (float)size_s;
    terms[6] = (float)(t[RC_CLS_POS] * w);
    terms[7] = (float)(t[RC_CLS_NEG] * w);
#pragma unroll
    for (int k = 0; k < 8; ++k) terms[8 + k] = (float)head[k];
    terms[16] = (float)loc;
    terms[17] = (float)angle;
    terms[18] = (float)size_mean;
#pragma unroll
    for (int k = 0; k < 4; ++k) terms[19 + k] = (float)counts[k];
}

template <bool BWD>
__global__ __launch_bounds__(RC_ROWS) void rcnn_loss_main_kernel(const RcParams P) {
    __shared__ float s_row[RC_ROWS * RC_LDC];
    __shared__ int s_cls[RC_ROWS], s_msk[RC_ROWS];
    __shared__ double s_red[RC_WAVES][RC_TERMS];
    __shared__ double s_tot[RC_TERMS];
    __shared__ int s_cnt[RC_WAVES][4];
    __shared__ int s_cnt_tot[4];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * RC_ROWS;
    const int rows = (int)(P.npts - row0 < RC_ROWS ? P.npts - row0 : RC_ROWS);
    const int C = P.cfg.C;
    const int ldc = C | 1;
    const int elems = rows * C;

    if (tid < rows) {
        s_cls[tid] = rc_sign(rc_int(P.label, P.label_i64, row0 + tid));
        s_msk[tid] = rc_sign(rc_int(P.mask, P.mask_i64, row0 + tid));
    }
    if (!BWD && blockIdx.x == 0) {                            // the integer counts over ALL rows
        int cnt[4] = {0, 0, 0, 0};
        for (int64_t r = tid; r < P.npts; r += RC_ROWS) {
            const int64_t l = rc_int(P.label, P.label_i64, r), m = rc_int(P.mask, P.mask_i64, r);
            cnt[0] += l > 0;
            cnt[1] += l >= 0;
            cnt[2] += m > 0;
            cnt[3] += (int)m;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int v = cnt[k];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
            if ((tid & 63) == 0) s_cnt[tid >> 6][k] = v;
        }
    }
    __syncthreads();
    if (!BWD && blockIdx.x == 0 && tid < 4) {
        int v = s_cnt[0][tid];
        for (int wv = 1; wv < RC_WAVES; ++wv) v += s_cnt[wv][tid];
        s_cnt_tot[tid] = v;
        P.counts[tid] = v;
    }
    for (int i = tid; i < elems; i += RC_ROWS) {
        const int r = i / C;
        if (s_msk[r] <= 0) continue;                          // not regressed: the row is never read
        const int c = i - r * C;
        s_row[r * ldc + c] = P.reg[(row0 + r) * P.ld_reg + c];
    }
    __syncthreads();

    double acc[RC_TERMS];
#pragma unroll
    for (int k = 0; k < RC_TERMS; ++k) acc[k] = 0.0;
    if (tid < rows) {
        const int l = s_cls[tid];
        float w = 1.0f, g_reg = 0.0f, go = 0.0f;
        if (BWD) {
            const int n_cls = P.cfg.loss_cls == RC_LOSS_FOCAL ? P.counts[0] : P.counts[1];
            const int fg = P.counts[2];
            go = P.grad_out[0];
            w = P.norm ? P.norm[0] : 1.0f / (float)(n_cls > 1 ? n_cls : 1);
            g_reg = (float)((double)go * (P.norm ? (double)P.norm[1] : 1.0) / (double)(fg > 1 ? fg : 1));
        }
        if (l >= 0) {
            const float x = P.cls[(row0 + tid) * P.ld_cls];
            const float t = l > 0 ? 1.0f : 0.0f;
            float v, dx;
            if (P.cfg.loss_cls == RC_LOSS_FOCAL) {
                rl_focal(x, t, w, P.cfg.xz, &v, &dx);
            } else {
                rc_bce(x, t, &v, &dx);
                dx = w * dx;
            }
            if (BWD) {
                P.dcls[row0 + tid] = go * dx;
            } else {
                acc[RC_CLS] = (double)v;
                if (l > 0) acc[RC_CLS_POS] = (double)v;
                else acc[RC_CLS_NEG] = (double)v;
            }
        } else if (BWD) {
            P.dcls[row0 + tid] = 0.0f;
        }
        if (s_msk[tid] > 0) {
            float lab[7], anchor[3];
            const float* gt = P.gt + (row0 + tid) * 7;
#pragma unroll
            for (int k = 0; k < 7; ++k) lab[k] = gt[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) anchor[k] = P.cfg.size_on_roi ? P.roi[(row0 + tid) * 7 + 3 + k] : P.cfg.xz.anchor[k];
            rc_reg_row<BWD, double>(&s_row[tid * ldc], lab, anchor, P.cfg, g_reg, acc);
        }
    }

    if (BWD) {
        __syncthreads();
        float* dst = P.dreg + row0 * C;
        for (int i = tid; i < elems; i += RC_ROWS) {
            const int r = i / C;
            dst[i] = s_msk[r] > 0 ? s_row[r * ldc + (i - r * C)] : 0.0f;
        }
    } else {
        // lanes of a wave: a fixed shuffle tree; waves: summed in order by the first RC_TERMS lanes
#pragma unroll
        for (int k = 0; k < RC_TERMS; ++k) {
            double v = acc[k];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
            if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
        }
        __syncthreads();
        const bool inline_finalize = P.finalize && gridDim.x == 1;
        if (tid < RC_TERMS) {
            double v = s_red[0][tid];
            for (int wv = 1; wv < RC_WAVES; ++wv) v += s_red[wv][tid];
            if (inline_finalize) s_tot[tid] = v;
            else P.partial[(int64_t)blockIdx.x * RC_TERMS + tid] = v;
        }
        if (inline_finalize) {
            __syncthreads();
            if (tid == 0) rc_finalize(s_tot, s_cnt_tot, nullptr, P.cfg, P.terms);
        }
    }
}

__global__ __launch_bounds__(RC_ROWS) void rcnn_loss_finalize_kernel(const double* __restrict__ partial, int blocks,
                                                                     const int32_t* __restrict__ counts, const float* __restrict__ norm,
                                                                     const RcConfig cfg, float* __restrict__ terms) {
    __shared__ double s_sum[RC_ROWS][RC_TERMS];
    const int tid = threadIdx.x;
    double acc[RC_TERMS];
#pragma unroll
    for (int k = 0; k < RC_TERMS; ++k) acc[k] = 0.0;
    for (int b = tid; b < blocks; b += RC_ROWS) {
#pragma unroll
        for (int k = 0; k < RC_TERMS; ++k) acc[k] += partial[(int64_t)b * RC_TERMS + k];
    }
#pragma unroll
    for (int k = 0; k < RC_TERMS; ++k) s_sum[tid][k] = acc[k];
    __syncthreads();
    for (int s = RC_ROWS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < RC_TERMS; ++k) s_sum[tid][k] += s_sum[tid + s][k];
        }
        __syncthreads();
    }
    if (tid == 0) rc_finalize(s_sum[0], counts, norm, cfg, terms);
}

// ------------------------------------------------------------------------------------------------ exports
static int rc_config(const char* who, const prcnn_rcnn_loss_cfg_t* cfg, int C, RcConfig* out) {
    if (!cfg) return prcnn_fail(PRCNN_EINVAL, "%s: null configuration", who);
    if (cfg->loss_cls != RC_LOSS_FOCAL && cfg->loss_cls != RC_LOSS_BCE)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: only SigmoidFocalLoss (loss_cls 0) and BinaryCrossEntropy (2) have a kernel, got %d", who,
                          cfg->loss_cls);
    if (cfg->loss_cls == RC_LOSS_FOCAL && !(cfg->gamma >= 0.0)) return prcnn_fail(PRCNN_EINVAL, "%s: focal gamma must be >= 0, got %g", who, cfg->gamma);
    if (!(cfg->loc_scope > 0.0) || !(cfg->loc_bin_size > 0.0) || cfg->num_head_bin < 1)
        return prcnn_fail(PRCNN_EINVAL, "%s: bad bins: scope %g, bin size %g, head bins %d", who, cfg->loc_scope, cfg->loc_bin_size, cfg->num_head_bin);
    if (cfg->y_by_bin && (!(cfg->loc_y_scope > 0.0) || !(cfg->loc_y_bin_size > 0.0)))
        return prcnn_fail(PRCNN_EINVAL, "%s: bad y bins: scope %g, bin size %g", who, cfg->loc_y_scope, cfg->loc_y_bin_size);
    const RcConfig c = rc_make_config(cfg->loc_scope, cfg->loc_bin_size, cfg->num_head_bin, cfg->y_by_bin != 0, cfg->y_by_bin ? cfg->loc_y_scope : 0.5,
                                      cfg->y_by_bin ? cfg->loc_y_bin_size : 0.25, cfg->size_res_on_roi != 0, cfg->mean_size, cfg->loss_cls,
                                      cfg->gamma, cfg->alpha, cfg->has_alpha != 0);
    if (c.xz.nb < 1 || c.xz.nb > RL_MAX_BINS || c.nh > RL_MAX_BINS || (c.y_by_bin && (c.y.nb < 1 || c.y.nb > RL_MAX_BINS)))
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: %d location bins / %d y bins / %d angle bins, the kernel holds 1 to %d", who, c.xz.nb,
                          c.y_by_bin ? c.y.nb : 0, c.nh, RL_MAX_BINS);
    if (C != c.C) return prcnn_fail(PRCNN_EINVAL, "%s: rcnn_reg has %d channels, the configuration describes %d", who, C, c.C);
    if (c.C > RC_MAX_C) return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: %d channels per row, the kernel holds at most %d", who, c.C, RC_MAX_C);
    *out = c;
    return PRCNN_OK;
}

static int rc_params(const char* who, const float* rcnn_cls, int64_t ld_cls, const float* rcnn_reg, int64_t ld_reg, const void* cls_label,
                     int label_is_i64, const void* reg_valid_mask, int mask_is_i64, const float* roi_boxes3d, const float* gt_of_rois,
                     int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, RcParams* P) {
    const int rc = rc_config(who, cfg, C, &P->cfg);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(npts >= 1, "%s: bad row count %lld", who, (long long)npts);
    if (npts > RC_MAX_ROWS) return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: %lld rows, the kernel takes at most %lld", who, (long long)npts, (long long)RC_MAX_ROWS);
    PRCNN_REQUIRE(ld_cls >= 1 && ld_reg >= C, "%s: bad row strides %lld / %lld for %d channels", who, (long long)ld_cls, (long long)ld_reg, C);
    PRCNN_REQUIRE(rcnn_cls && rcnn_reg && cls_label && reg_valid_mask && gt_of_rois && (roi_boxes3d || !cfg->size_res_on_roi), "%s: null pointer", who);
    P->cls = rcnn_cls;
    P->reg = rcnn_reg;
    P->ld_cls = ld_cls;
    P->ld_reg = ld_reg;
    P->label = cls_label;
    P->mask = reg_valid_mask;
    P->label_i64 = label_is_i64 != 0;
    P->mask_i64 = mask_is_i64 != 0;
    P->roi = roi_boxes3d;
    P->gt = gt_of_rois;
    P->npts = npts;
    P->norm = nullptr;
    P->counts = nullptr;
    P->grad_out = nullptr;
    P->dcls = nullptr;
    P->dreg = nullptr;
    P->partial = nullptr;
    P->terms = nullptr;
    P->finalize = 0;
    return PRCNN_OK;
}

PRCNN_API size_t prcnn_rcnn_loss_workspace_bytes(int64_t npts) {
    if (npts < 0 || npts > RC_MAX_ROWS) return 0;
    return (size_t)rc_blocks(npts) * RC_TERMS * sizeof(double) + 16;
}

static int rc_work_ok(const char* who, int64_t npts, const void* work, size_t work_bytes) {
    PRCNN_REQUIRE(work && work_bytes >= prcnn_rcnn_loss_workspace_bytes(npts) && (uintptr_t)work % 8 == 0,
                  "%s: workspace of %zu bytes, need %zu (8-byte aligned)", who, work_bytes, prcnn_rcnn_loss_workspace_bytes(npts));
    return PRCNN_OK;
}

PRCNN_API int prcnn_rcnn_loss_forward(const float* rcnn_cls, int64_t ld_cls, const float* rcnn_reg, int64_t ld_reg, const void* cls_label,
                                      int label_is_i64, const void* reg_valid_mask, int mask_is_i64, const float* roi_boxes3d,
                                      const float* gt_of_rois, int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, int finalize,
                                      int32_t* counts, float* terms, void* work, size_t work_bytes, prcnn_stream_t stream) {
    RcParams P;
    int rc = rc_params("prcnn_rcnn_loss_forward", rcnn_cls, ld_cls, rcnn_reg, ld_reg, cls_label, label_is_i64, reg_valid_mask, mask_is_i64,
                       roi_boxes3d, gt_of_rois, npts, C, cfg, &P);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(counts && (terms || !finalize), "prcnn_rcnn_loss_forward: null pointer");
    rc = rc_work_ok("prcnn_rcnn_loss_forward", npts, work, work_bytes);
    if (rc != PRCNN_OK) return rc;
    P.counts = counts;
    P.terms = terms;
    P.partial = (double*)work;
    P.finalize = finalize != 0;
    const int blocks = rc_blocks(npts);
    hipLaunchKernelGGL(rcnn_loss_main_kernel<false>, dim3(blocks), dim3(RC_ROWS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_rcnn_loss_forward");
    if (finalize && blocks > 1) {
        hipLaunchKernelGGL(rcnn_loss_finalize_kernel, dim3(1), dim3(RC_ROWS), 0, (hipStream_t)stream, (const double*)work, blocks,
                           (const int32_t*)counts, (const float*)nullptr, P.cfg, terms);
        PRCNN_LAUNCH_CHECK("prcnn_rcnn_loss_forward");
    }
    return PRCNN_OK;
}

PRCNN_API int prcnn_rcnn_loss_finalize(int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, const int32_t* counts, const float* norm,
                                       float* terms, const void* work, size_t work_bytes, prcnn_stream_t stream) {
    RcConfig c;
    int rc = rc_config("prcnn_rcnn_loss_finalize", cfg, C, &c);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(npts >= 1 && npts <= RC_MAX_ROWS, "prcnn_rcnn_loss_finalize: bad row count %lld", (long long)npts);
    PRCNN_REQUIRE(counts && terms, "prcnn_rcnn_loss_finalize: null pointer");
    rc = rc_work_ok("prcnn_rcnn_loss_finalize", npts, work, work_bytes);
    if (rc != PRCNN_OK) return rc;
    hipLaunchKernelGGL(rcnn_loss_finalize_kernel, dim3(1), dim3(RC_ROWS), 0, (hipStream_t)stream, (const double*)work, rc_blocks(npts), counts,
                       norm, c, terms);
    PRCNN_LAUNCH_CHECK("prcnn_rcnn_loss_finalize");
    return PRCNN_OK;
}

PRCNN_API int prcnn_rcnn_loss_backward(const float* rcnn_cls, int64_t ld_cls, const float* rcnn_reg, int64_t ld_reg, const void* cls_label,
                                       int label_is_i64, const void* reg_valid_mask, int mask_is_i64, const float* roi_boxes3d,
                                       const float* gt_of_rois, int64_t npts, int C, const prcnn_rcnn_loss_cfg_t* cfg, const int32_t* counts,
                                       const float* norm, const float* grad_out, float* dcls, float* dreg, prcnn_stream_t stream) {
    RcParams P;
    const int rc = rc_params("prcnn_rcnn_loss_backward", rcnn_cls, ld_cls, rcnn_reg, ld_reg, cls_label, label_is_i64, reg_valid_mask,
                             mask_is_i64, roi_boxes3d, gt_of_rois, npts, C, cfg, &P);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(counts && grad_out && dcls && dreg, "prcnn_rcnn_loss_backward: null pointer");
    P.counts = const_cast<int32_t*>(counts);
    P.norm = norm;
    P.grad_out = grad_out;
    P.dcls = dcls;
    P.dreg = dreg;
    hipLaunchKernelGGL(rcnn_loss_main_kernel<true>, dim3(rc_blocks(npts)), dim3(RC_ROWS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_rcnn_loss_backward");
    return PRCNN_OK;
}
