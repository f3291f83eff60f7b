// rpn_loss.hip -- the RPN training loss (train_functions.get_rpn_loss) and its gradient on the device: SigmoidFocalLoss, DiceLoss
// or BinaryCrossEntropy classification + bin-based box regression over the foreground rows (arithmetic: rpn_loss_math.h).
//
//   prcnn_rpn_loss_counts    pos = #(label > 0), valid = #(label >= 0), fg = pos as integers: per-workgroup partial counts, summed by one
//                            workgroup in a fixed order.  It also writes the single-process normalisers {1 / max(pos, 1), 1}; a
//                            data-parallel caller all-reduces the counts and overwrites them with {world / max(pos_global, 1),
//                            world * fg_local / max(fg_global, 1)}.  The other two exports read counts and normalisers from the device.
//   prcnn_rpn_loss_forward   one launch over all rows (RL_ROWS rows per workgroup, one lane per row): the focal term of every valid row,
//                            the eight regression terms of every foreground row, summed per workgroup in double in a fixed order;
//                            then one workgroup sums the partials in a fixed order, applies the means (divisor count x columns; an
//                            empty selection gives 0), 3 x size, the data-parallel scale and LOSS_WEIGHT and writes 9 floats.
//   prcnn_rpn_loss_backward  the same launch geometry with grad_output read from the device: d loss / d rpn_cls and d loss / d rpn_reg,
//                            every entry written exactly once (no memset, no atomics).
// The three exports above are SigmoidFocalLoss only.  All three RPN.LOSS_CLS kinds go through
//   prcnn_rpn_loss_cls_sums       DiceLoss only: A = sum min(p, t), B = sum max(p, t) over the valid rows, per-workgroup partials in
//                                 double, summed by one workgroup in a fixed order into two doubles on the device (a data-parallel
//                                 caller all-reduces them in place before the next two calls)
//   prcnn_rpn_loss_forward_kind   the forward launches with the kind's classification term: focal as above; BCE row terms summed into
//                                 the same slot and scaled by norm[0] at the end; Dice formed as 1 - A / max(B, 1) from the two doubles
//   prcnn_rpn_loss_backward_kind  the backward launch; Dice reads A and B from the device
// with norm NULL (Dice, BCE) standing for the single-process normalisers {Dice 1 | BCE 1 / max(valid, 1), 1}.
// The regression row of a row that is not foreground is never read: only foreground rows are staged (16-byte units, coalesced) into
// LDS, where the row's lane works on them in place; the gradient tile leaves LDS in 16-byte units again, zeros for the other rows.
// The grid is a function of the row count alone, and no result depends on anything but the rows in their flat order.
#include "common.h"
#include "rpn_loss_math.h"

constexpr int RL_ROWS = 128;              // rows per workgroup
constexpr int RL_THREADS = 256;
constexpr int RL_MAX_C = 96;              // widest regression row held in LDS (C = 76 / 52 for the stock heads); ops.RPN_LOSS_MAX_C
constexpr int RL_CNT_THREADS = 256;
constexpr int RL_CNT_PER_THREAD = 8;
constexpr int RL_CNT_MAX_BLOCKS = 1024;

static inline int rl_main_blocks(int64_t npts) { return (int)((npts + RL_ROWS - 1) / RL_ROWS); }
static inline int rl_count_blocks(int64_t npts) {
    const int64_t per = (int64_t)RL_CNT_THREADS * RL_CNT_PER_THREAD;
    const int64_t b = (npts + per - 1) / per;
    return (int)(b < 1 ? 1 : (b > RL_CNT_MAX_BLOCKS ? RL_CNT_MAX_BLOCKS : b));
}
static inline size_t rl_partial_bytes(int64_t npts) { return (size_t)rl_main_blocks(npts) * RL_TERMS * sizeof(double); }

__device__ __forceinline__ int rl_label(const void* label, int is_i64, int64_t r) {
    if (is_i64) {
        const int64_t v = ((const int64_t*)label)[r];
        return v > 0 ? 1 : (v == 0 ? 0 : -1);
    }
    const int32_t v = ((const int32_t*)label)[r];
    return v > 0 ? 1 : (v == 0 ? 0 : -1);
}

// ------------------------------------------------------------------------------------------------ counts
__global__ __launch_bounds__(RL_CNT_THREADS) void rpn_loss_count_kernel(const void* __restrict__ label, int is_i64, int64_t npts,
                                                                        int32_t* __restrict__ part) {
    __shared__ int s_pos[RL_CNT_THREADS], s_valid[RL_CNT_THREADS];
    int pos = 0, valid = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < npts; r += (int64_t)gridDim.x * blockDim.x) {
        const int l = rl_label(label, is_i64, r);
        pos += l > 0;
        valid += l >= 0;
    }
    s_pos[threadIdx.x] = pos;
    s_valid[threadIdx.x] = valid;
    __syncthreads();
    for (int s = RL_CNT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_pos[threadIdx.x] += s_pos[threadIdx.x + s];
            s_valid[threadIdx.x] += s_valid[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x + 0] = s_pos[0];
        part[2 * blockIdx.x + 1] = s_valid[0];
    }
}

__global__ __launch_bounds__(RL_CNT_THREADS) void rpn_loss_count_sum_kernel(const int32_t* __restrict__ part, int blocks,
                                                                            int32_t* __restrict__ counts, float* __restrict__ norm) {
    __shared__ int s_pos[RL_CNT_THREADS], s_valid[RL_CNT_THREADS];
    int pos = 0, valid = 0;
    for (int b = threadIdx.x; b < blocks; b += RL_CNT_THREADS) {
        pos += part[2 * b + 0];
        valid += part[2 * b + 1];
    }
    s_pos[threadIdx.x] = pos;
    s_valid[threadIdx.x] = valid;
    __syncthreads();
    for (int s = RL_CNT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_pos[threadIdx.x] += s_pos[threadIdx.x + s];
            s_valid[threadIdx.x] += s_valid[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        counts[0] = s_pos[0];
        counts[1] = s_valid[0];
        counts[2] = s_pos[0];
        counts[3] = 0;
        norm[0] = 1.0f / (float)(s_pos[0] > 1 ? s_pos[0] : 1);
        norm[1] = 1.0f;
    }
}

// ------------------------------------------------------------------------------------------------ Dice sums
// A = sum min(p, t), B = sum max(p, t) over the valid rows: the geometry of the counts, float32 addends summed in double
__global__ __launch_bounds__(RL_CNT_THREADS) void rpn_loss_dice_kernel(const float* __restrict__ cls, int64_t ld_cls,
                                                                       const void* __restrict__ label, int is_i64, int64_t npts,
                                                                       double* __restrict__ part) {
    __shared__ double s_a[RL_CNT_THREADS], s_b[RL_CNT_THREADS];
    double a = 0.0, b = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < npts; r += (int64_t)gridDim.x * blockDim.x) {
        const int l = rl_label(label, is_i64, r);
        if (l < 0) continue;
        float lo, hi, dlo, dhi;
        rl_dice(cls[r * ld_cls], (float)l, &lo, &hi, &dlo, &dhi);
        a += (double)lo;
        b += (double)hi;
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (int s = RL_CNT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_a[threadIdx.x] += s_a[threadIdx.x + s];
            s_b[threadIdx.x] += s_b[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x + 0] = s_a[0];
        part[2 * blockIdx.x + 1] = s_b[0];
    }
}

__global__ __launch_bounds__(RL_CNT_THREADS) void rpn_loss_dice_sum_kernel(const double* __restrict__ part, int blocks,
                                                                           double* __restrict__ sums) {
    __shared__ double s_a[RL_CNT_THREADS], s_b[RL_CNT_THREADS];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < blocks; i += RL_CNT_THREADS) {
        a += part[2 * i + 0];
        b += part[2 * i + 1];
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (int s = RL_CNT_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            s_a[threadIdx.x] += s_a[threadIdx.x + s];
            s_b[threadIdx.x] += s_b[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        sums[0] = s_a[0];
        sums[1] = s_b[0];
    }
}

// ------------------------------------------------------------------------------------------------ main pass
struct RlParams {
    const float* cls;           // row r's logit at cls[r * ld_cls]
    const float* reg;           // row r's C predictions at reg + r * ld_reg
    int64_t ld_cls, ld_reg;
    const void* label;          // (npts) i32 or i64
    int label_i64;
    int vec;                    // reg rows can be read in 16-byte units
    const float* reg_label;     // (npts, 7)
    int64_t npts;
    const int32_t* counts;      // local {pos, valid, fg, 0}
    const float* norm;          // {cls weight, regression scale}
    const float* grad_out;      // backward: the upstream scalar
    float* dcls;                // backward: (npts)
    float* dreg;                // backward: (npts, C) contiguous
    double* partial;            // forward: (blocks, RL_TERMS)
    RlConfig cfg;
    const double* cls_sums;     // Dice: {A, B}
    float fg_weight;            // BCE: the weight of a foreground row
};

// the classification (k = 0) or regression (k = 1) normaliser; Dice and BCE accept norm == NULL: the single-process values
template <int KIND>
__device__ __forceinline__ float rl_norm(const float* norm, const int32_t* counts, int k) {
    if (KIND == RL_KIND_FOCAL || norm) return norm[k];
    if (k == 1 || KIND == RL_KIND_DICE) return 1.0f;
    const int valid = counts[1];
    return 1.0f / (float)(valid > 1 ? valid : 1);
}

template <bool BWD, int KIND>
__global__ __launch_bounds__(RL_THREADS) void rpn_loss_main_kernel(const RlParams P) {
    __shared__ __attribute__((aligned(16))) float s_row[RL_ROWS * RL_MAX_C];
    __shared__ float s_lab[RL_ROWS * 7];
    __shared__ int s_cls[RL_ROWS];
    __shared__ double s_red[RL_THREADS / 64][RL_TERMS];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * RL_ROWS;
    const int rows = (int)(P.npts - row0 < RL_ROWS ? P.npts - row0 : RL_ROWS);
    const int C = P.cfg.C;
    const int upr = C >> 2;                                   // 16-byte units per row
    const int units = rows * upr;

    if (tid < rows) s_cls[tid] = rl_label(P.label, P.label_i64, row0 + tid);
    for (int i = tid; i < rows * 7; i += RL_THREADS) s_lab[i] = P.reg_label[row0 * 7 + i];
    __syncthreads();
    for (int u = tid; u < units; u += RL_THREADS) {
        const int r = u / upr;
        if (s_cls[r] <= 0) continue;                          // not foreground: the row is never read
        const int c4 = (u - r * upr) << 2;
        const float* src = P.reg + (row0 + r) * P.ld_reg + c4;
        float4 v;
        if (P.vec) {
            v = *(const float4*)src;
        } else {
            v.x = src[0];
            v.y = src[1];
            v.z = src[2];
            v.w = src[3];
        }
        *(float4*)&s_row[4 * u] = v;
    }
    __syncthreads();

    double acc[RL_TERMS];
#pragma unroll
    for (int k = 0; k < RL_TERMS; ++k) acc[k] = 0.0;
    if (tid < rows) {
        const int l = s_cls[tid];
        const float w = rl_norm<KIND>(P.norm, P.counts, 0);
        float g_cls = 0.0f, g_reg = 0.0f;
        if (BWD) {
            const double go = (double)P.grad_out[0];
            const int fg = P.counts[2];
            g_cls = (float)(go * P.cfg.w_cls);
            g_reg = (float)(go * P.cfg.w_reg * (double)rl_norm<KIND>(P.norm, P.counts, 1) / (double)(fg > 1 ? fg : 1));
        }
        if (KIND == RL_KIND_FOCAL) {
            if (l >= 0) {
                float v, dx;
                rl_focal(P.cls[(row0 + tid) * P.ld_cls], (float)l, w, P.cfg, &v, &dx);
                if (BWD) {
                    P.dcls[row0 + tid] = g_cls * dx;
                } else {
                    acc[RL_CLS] = (double)v;
                    if (l > 0) acc[RL_CLS_POS] = (double)v;
                    else acc[RL_CLS_NEG] = (double)v;
                }
            } else if (BWD) {
                P.dcls[row0 + tid] = 0.0f;
            }
        } else if (KIND == RL_KIND_BCE) {
            // the row terms are summed unscaled; norm[0] multiplies the sum (finalize) and the upstream gradient
            float v, dx;
            rl_bce_row(P.cls[(row0 + tid) * P.ld_cls], l, P.fg_weight, &v, &dx);
            if (BWD) P.dcls[row0 + tid] = l >= 0 ? (float)((double)g_cls * (double)w) * dx : 0.0f;
            else acc[RL_CLS] = (double)v;
        } else if (BWD) {
            // Dice: the (global) sums of the sums pass give every row's derivative; the forward pass has no row term
            float lo, hi, dlo, dhi;
            rl_dice_row(P.cls[(row0 + tid) * P.ld_cls], l, &lo, &hi, &dlo, &dhi);
            P.dcls[row0 + tid] = l >= 0 ? rl_dice_grad(dlo, dhi, P.cls_sums[0], P.cls_sums[1], (double)g_cls * (double)w) : 0.0f;
        }
        if (l > 0) rl_reg_row<BWD, double>(&s_row[tid * C], &s_lab[tid * 7], P.cfg, g_reg, acc);
    }

    if (BWD) {
        __syncthreads();
        float4* dst = (float4*)(P.dreg + row0 * C);
        for (int u = tid; u < units; u += RL_THREADS) {
            const int r = u / upr;
            dst[u] = s_cls[r] > 0 ? *(const float4*)&s_row[4 * u] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    } else {
        // lanes of a wave: a fixed shuffle tree; waves: summed in order by the first RL_TERMS lanes
#pragma unroll
        for (int k = 0; k < RL_TERMS; ++k) {
            double v = acc[k];
            for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
            if ((tid & 63) == 0) s_red[tid >> 6][k] = v;
        }
        __syncthreads();
        if (tid < RL_TERMS) {
            double v = s_red[0][tid];
            for (int wv = 1; wv < RL_THREADS / 64; ++wv) v += s_red[wv][tid];
            P.partial[(int64_t)blockIdx.x * RL_TERMS + tid] = v;
        }
    }
}

// sums the per-workgroup partials in a fixed order and forms the named terms (doubles, rounded to float once at the end)
template <int KIND>
__global__ __launch_bounds__(RL_THREADS) void rpn_loss_finalize_kernel(const double* __restrict__ partial, int blocks,
                                                                       const int32_t* __restrict__ counts, const float* __restrict__ norm,
                                                                       const RlConfig cfg, const double* __restrict__ cls_sums,
                                                                       float* __restrict__ terms) {
    __shared__ double s_sum[RL_THREADS][RL_TERMS];
    const int tid = threadIdx.x;
    double acc[RL_TERMS];
#pragma unroll
    for (int k = 0; k < RL_TERMS; ++k) acc[k] = 0.0;
    for (int b = tid; b < blocks; b += RL_THREADS) {
#pragma unroll
        for (int k = 0; k < RL_TERMS; ++k) acc[k] += partial[(int64_t)b * RL_TERMS + k];
    }
#pragma unroll
    for (int k = 0; k < RL_TERMS; ++k) s_sum[tid][k] = acc[k];
    __syncthreads();
    for (int s = RL_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) {
            for (int k = 0; k < RL_TERMS; ++k) s_sum[tid][k] += s_sum[tid + s][k];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double* t = s_sum[0];
        const int fg = counts[2];
        const double cnt = (double)(fg > 1 ? fg : 1);
        const double scale = (double)rl_norm<KIND>(norm, counts, 1);
        double loc = t[RL_X_BIN] / cnt + t[RL_Z_BIN] / cnt + t[RL_Y_OFF] / cnt;
        if (cfg.xz_fine) loc += t[RL_X_RES] / cnt + t[RL_Z_RES] / cnt;
        double angle = t[RL_RY_BIN] / cnt + t[RL_RY_RES] / cnt;
        double size = 3.0 * (t[RL_SIZE] / (cnt * 3.0));
        loc *= scale;
        angle *= scale;
        size *= scale;
        const double reg = loc + angle + size;
        double cls = t[RL_CLS];
        if (KIND == RL_KIND_BCE) cls *= (double)rl_norm<KIND>(norm, counts, 0);
        if (KIND == RL_KIND_DICE) cls = 1.0 - cls_sums[0] / (cls_sums[1] > 1.0 ? cls_sums[1] : 1.0);
        terms[0] = (float)(cls * cfg.w_cls + reg * cfg.w_reg);
        terms[1] = (float)cls;
        terms[2] = (float)reg;
        terms[3] = (float)loc;
        terms[4] = (float)angle;
        terms[5] = (float)size;
        terms[6] = (float)t[RL_CLS_POS];
        terms[7] = (float)t[RL_CLS_NEG];
        terms[8] = (float)fg;
    }
}

// ------------------------------------------------------------------------------------------------ exports
// all_kinds: the *_kind exports take every RPN.LOSS_CLS; the first three exports are SigmoidFocalLoss only and say so
static int rl_config(const char* who, const prcnn_rpn_loss_cfg_t* cfg, int C, bool all_kinds, RlConfig* out) {
    if (!cfg) return prcnn_fail(PRCNN_EINVAL, "%s: null configuration", who);
    if (!all_kinds && cfg->loss_cls != 0)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: only SigmoidFocalLoss (loss_cls 0) has a kernel, got %d", who, cfg->loss_cls);
    if (cfg->loss_cls < RL_KIND_FOCAL || cfg->loss_cls > RL_KIND_BCE)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: loss_cls %d is none of SigmoidFocalLoss (0), DiceLoss (1), BinaryCrossEntropy (2)", who, cfg->loss_cls);
    if (cfg->y_by_bin || cfg->ry_fine) return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: get_y_by_bin / get_ry_fine have no kernel", who);
    if (cfg->loss_cls == RL_KIND_FOCAL && !(cfg->gamma >= 0.0)) return prcnn_fail(PRCNN_EINVAL, "%s: focal gamma must be >= 0, got %g", who, cfg->gamma);
    if (!(cfg->loc_scope > 0.0) || !(cfg->loc_bin_size > 0.0) || cfg->num_head_bin < 1)
        return prcnn_fail(PRCNN_EINVAL, "%s: bad bins: scope %g, bin size %g, head bins %d", who, cfg->loc_scope, cfg->loc_bin_size, cfg->num_head_bin);
    const RlConfig c = rl_make_config(cfg->loc_scope, cfg->loc_bin_size, cfg->num_head_bin, cfg->xz_fine != 0, cfg->mean_size, cfg->gamma,
                                      cfg->alpha, cfg->has_alpha != 0, cfg->loss_weight[0], cfg->loss_weight[1]);
    if (c.nb < 1 || c.nb > RL_MAX_BINS || c.nh > RL_MAX_BINS)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: %d location bins / %d angle bins, the kernel holds at most %d", who, c.nb, c.nh, RL_MAX_BINS);
    if (C != c.C) return prcnn_fail(PRCNN_EINVAL, "%s: rpn_reg has %d channels, the configuration describes %d", who, C, c.C);
    if (c.C % 4 != 0 || c.C > RL_MAX_C)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: %d channels per row: the kernel needs a multiple of 4 up to %d", who, c.C, RL_MAX_C);
    *out = c;
    return PRCNN_OK;
}

static int rl_params(const char* who, const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                     int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg, const int32_t* counts,
                     const float* norm, bool all_kinds, const double* cls_sums, double fg_weight, RlParams* P) {
    const int rc = rl_config(who, cfg, C, all_kinds, &P->cfg);
    if (rc != PRCNN_OK) return rc;
    const int kind = cfg->loss_cls;
    PRCNN_REQUIRE(npts >= 0 && npts < ((int64_t)1 << 31) * RL_ROWS, "%s: bad row count %lld", who, (long long)npts);
    PRCNN_REQUIRE(ld_cls >= 1 && ld_reg >= C, "%s: bad row strides %lld / %lld for %d channels", who, (long long)ld_cls, (long long)ld_reg, C);
    if (npts > 0)
        PRCNN_REQUIRE(rpn_cls && rpn_reg && cls_label && reg_label && counts && (norm || kind != RL_KIND_FOCAL), "%s: null pointer", who);
    if (kind == RL_KIND_DICE) PRCNN_REQUIRE(cls_sums && (uintptr_t)cls_sums % 8 == 0, "%s: DiceLoss needs the two sums of prcnn_rpn_loss_cls_sums", who);
    if (kind == RL_KIND_BCE) PRCNN_REQUIRE(std::isfinite(fg_weight), "%s: FG_WEIGHT must be finite, got %g", who, fg_weight);
    P->cls = rpn_cls;
    P->reg = rpn_reg;
    P->ld_cls = ld_cls;
    P->ld_reg = ld_reg;
    P->label = cls_label;
    P->label_i64 = label_is_i64 != 0;
    P->vec = ((uintptr_t)rpn_reg % 16 == 0) && (ld_reg % 4 == 0);
    P->reg_label = reg_label;
    P->npts = npts;
    P->counts = counts;
    P->norm = norm;
    P->grad_out = nullptr;
    P->dcls = nullptr;
    P->dreg = nullptr;
    P->partial = nullptr;
    P->cls_sums = kind == RL_KIND_DICE ? cls_sums : nullptr;
    P->fg_weight = (float)fg_weight;
    return PRCNN_OK;
}

PRCNN_API size_t prcnn_rpn_loss_workspace_bytes(int64_t npts) {
    if (npts < 0) return 0;
    const size_t cnt = (size_t)rl_count_blocks(npts) * 2 * sizeof(double);     // the Dice partials; the counts' are half of it
    const size_t sum = rl_partial_bytes(npts);
    return (cnt > sum ? cnt : sum) + 16;
}

PRCNN_API int prcnn_rpn_loss_counts(const void* cls_label, int label_is_i64, int64_t npts, int32_t* counts, float* norm, void* work,
                                    size_t work_bytes, prcnn_stream_t stream) {
    PRCNN_REQUIRE(npts >= 0, "prcnn_rpn_loss_counts: bad row count %lld", (long long)npts);
    PRCNN_REQUIRE(counts && norm && work && (cls_label || npts == 0), "prcnn_rpn_loss_counts: null pointer");
    PRCNN_REQUIRE(work_bytes >= prcnn_rpn_loss_workspace_bytes(npts) && (uintptr_t)work % 8 == 0,
                  "prcnn_rpn_loss_counts: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, prcnn_rpn_loss_workspace_bytes(npts));
    const int blocks = rl_count_blocks(npts);
    hipLaunchKernelGGL(rpn_loss_count_kernel, dim3(blocks), dim3(RL_CNT_THREADS), 0, (hipStream_t)stream, cls_label, label_is_i64 != 0, npts,
                       (int32_t*)work);
    PRCNN_LAUNCH_CHECK("prcnn_rpn_loss_counts");
    hipLaunchKernelGGL(rpn_loss_count_sum_kernel, dim3(1), dim3(RL_CNT_THREADS), 0, (hipStream_t)stream, (const int32_t*)work, blocks, counts,
                       norm);
    PRCNN_LAUNCH_CHECK("prcnn_rpn_loss_counts");
    return PRCNN_OK;
}

PRCNN_API int prcnn_rpn_loss_cls_sums(const float* rpn_cls, int64_t ld_cls, const void* cls_label, int label_is_i64, int64_t npts,
                                      double* cls_sums, void* work, size_t work_bytes, prcnn_stream_t stream) {
    PRCNN_REQUIRE(npts >= 0 && ld_cls >= 1, "prcnn_rpn_loss_cls_sums: bad row count %lld / stride %lld", (long long)npts, (long long)ld_cls);
    PRCNN_REQUIRE(cls_sums && work && ((rpn_cls && cls_label) || npts == 0), "prcnn_rpn_loss_cls_sums: null pointer");
    PRCNN_REQUIRE((uintptr_t)cls_sums % 8 == 0, "prcnn_rpn_loss_cls_sums: the two sums must be 8-byte aligned");
    PRCNN_REQUIRE(work_bytes >= prcnn_rpn_loss_workspace_bytes(npts) && (uintptr_t)work % 8 == 0,
                  "prcnn_rpn_loss_cls_sums: workspace of %zu bytes, need %zu (8-byte aligned)", work_bytes, prcnn_rpn_loss_workspace_bytes(npts));
    const int blocks = rl_count_blocks(npts);
    hipLaunchKernelGGL(rpn_loss_dice_kernel, dim3(blocks), dim3(RL_CNT_THREADS), 0, (hipStream_t)stream, rpn_cls, ld_cls, cls_label,
                       label_is_i64 != 0, npts, (double*)work);
    PRCNN_LAUNCH_CHECK("prcnn_rpn_loss_cls_sums");
    hipLaunchKernelGGL(rpn_loss_dice_sum_kernel, dim3(1), dim3(RL_CNT_THREADS), 0, (hipStream_t)stream, (const double*)work, blocks, cls_sums);
    PRCNN_LAUNCH_CHECK("prcnn_rpn_loss_cls_sums");
    return PRCNN_OK;
}

template <int KIND>
static int rl_launch_forward(const char* who, const RlParams& P, const double* work, float* terms, hipStream_t stream) {
    const int blocks = rl_main_blocks(P.npts);
    if (blocks > 0) {
        hipLaunchKernelGGL((rpn_loss_main_kernel<false, KIND>), dim3(blocks), dim3(RL_THREADS), 0, stream, P);
        PRCNN_LAUNCH_CHECK(who);
    }
    hipLaunchKernelGGL(rpn_loss_finalize_kernel<KIND>, dim3(1), dim3(RL_THREADS), 0, stream, work, blocks, P.counts, P.norm, P.cfg, P.cls_sums,
                       terms);
    PRCNN_LAUNCH_CHECK(who);
    return PRCNN_OK;
}

static int rl_forward(const char* who, const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                      int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg, const int32_t* counts,
                      const float* norm, float* terms, void* work, size_t work_bytes, bool all_kinds, const double* cls_sums, double fg_weight,
                      prcnn_stream_t stream) {
    RlParams P;
    const int rc = rl_params(who, rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts, norm, all_kinds,
                             cls_sums, fg_weight, &P);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(terms && work && counts && (norm || cfg->loss_cls != RL_KIND_FOCAL), "%s: null pointer", who);
    PRCNN_REQUIRE(work_bytes >= prcnn_rpn_loss_workspace_bytes(npts) && (uintptr_t)work % 8 == 0,
                  "%s: workspace of %zu bytes, need %zu (8-byte aligned)", who, work_bytes, prcnn_rpn_loss_workspace_bytes(npts));
    P.partial = (double*)work;
    if (cfg->loss_cls == RL_KIND_DICE) return rl_launch_forward<RL_KIND_DICE>(who, P, (const double*)work, terms, (hipStream_t)stream);
    if (cfg->loss_cls == RL_KIND_BCE) return rl_launch_forward<RL_KIND_BCE>(who, P, (const double*)work, terms, (hipStream_t)stream);
    return rl_launch_forward<RL_KIND_FOCAL>(who, P, (const double*)work, terms, (hipStream_t)stream);
}

static int rl_backward(const char* who, const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                       int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg, const int32_t* counts,
                       const float* norm, const float* grad_out, float* dcls, float* dreg, bool all_kinds, const double* cls_sums,
                       double fg_weight, prcnn_stream_t stream) {
    RlParams P;
    const int rc = rl_params(who, rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts, norm, all_kinds,
                             cls_sums, fg_weight, &P);
    if (rc != PRCNN_OK) return rc;
    if (npts == 0) return PRCNN_OK;
    PRCNN_REQUIRE(grad_out && dcls && dreg, "%s: null pointer", who);
    PRCNN_REQUIRE((uintptr_t)dreg % 16 == 0, "%s: the rpn_reg gradient must be 16-byte aligned", who);
    P.grad_out = grad_out;
    P.dcls = dcls;
    P.dreg = dreg;
    const dim3 grid(rl_main_blocks(npts));
    if (cfg->loss_cls == RL_KIND_DICE)
        hipLaunchKernelGGL((rpn_loss_main_kernel<true, RL_KIND_DICE>), grid, dim3(RL_THREADS), 0, (hipStream_t)stream, P);
    else if (cfg->loss_cls == RL_KIND_BCE)
        hipLaunchKernelGGL((rpn_loss_main_kernel<true, RL_KIND_BCE>), grid, dim3(RL_THREADS), 0, (hipStream_t)stream, P);
    else
        hipLaunchKernelGGL((rpn_loss_main_kernel<true, RL_KIND_FOCAL>), grid, dim3(RL_THREADS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK(who);
    return PRCNN_OK;
}

PRCNN_API int prcnn_rpn_loss_forward(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                     int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                     const int32_t* counts, const float* norm, float* terms, void* work, size_t work_bytes,
                                     prcnn_stream_t stream) {
    return rl_forward("prcnn_rpn_loss_forward", rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts, norm,
                      terms, work, work_bytes, false, nullptr, 1.0, stream);
}

PRCNN_API int prcnn_rpn_loss_backward(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                      int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                      const int32_t* counts, const float* norm, const float* grad_out, float* dcls, float* dreg,
                                      prcnn_stream_t stream) {
    return rl_backward("prcnn_rpn_loss_backward", rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts, norm,
                       grad_out, dcls, dreg, false, nullptr, 1.0, stream);
}

PRCNN_API int prcnn_rpn_loss_forward_kind(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                          int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                          const int32_t* counts, const float* norm, float* terms, void* work, size_t work_bytes,
                                          const double* cls_sums, double fg_weight, prcnn_stream_t stream) {
    return rl_forward("prcnn_rpn_loss_forward_kind", rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts,
                      norm, terms, work, work_bytes, true, cls_sums, fg_weight, stream);
}

PRCNN_API int prcnn_rpn_loss_backward_kind(const float* rpn_cls, int64_t ld_cls, const float* rpn_reg, int64_t ld_reg, const void* cls_label,
                                           int label_is_i64, const float* reg_label, int64_t npts, int C, const prcnn_rpn_loss_cfg_t* cfg,
                                           const int32_t* counts, const float* norm, const float* grad_out, float* dcls, float* dreg,
                                           const double* cls_sums, double fg_weight, prcnn_stream_t stream) {
    return rl_backward("prcnn_rpn_loss_backward_kind", rpn_cls, ld_cls, rpn_reg, ld_reg, cls_label, label_is_i64, reg_label, npts, C, cfg, counts,
                       norm, grad_out, dcls, dreg, true, cls_sums, fg_weight, stream);
}

