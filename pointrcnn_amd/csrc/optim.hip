// optim.hip -- the adam_onecycle parameter update (pointrcnn_amd/optim.py OneCycleAdam; arithmetic: optim_math.h) over ALL parameter
// tensors in two launches, whatever their number: gradient-norm clip, decoupled decay, Adam.
//
// Both kernels walk two device-resident tables the caller builds: one row per tensor {param, grad, exp_avg, exp_avg_sq, numel} and one
// row per chunk {tensor, first element}; a chunk is at most OPT_CHUNK consecutive elements of one tensor and belongs to one workgroup
// of 256 lanes.  Element j of a chunk is lane (j / 4) % 256's, whatever the alignment, so no result depends on which path read it.
//
//   prcnn_optim_grad_norm   partial[c] = sum of g^2 over chunk c in float64: each lane adds its elements in increasing order, the
//                           lanes of a wave fold in a fixed shuffle tree, the four waves are added in order.  Every slot is written
//                           (0 for a tensor without gradient): no atomics, no memset, the same bytes from the same state.
//   prcnn_optim_step        EVERY workgroup sums all partials itself -- lane l the contiguous slice [l * per, (l + 1) * per) in index
//                           order, then the same tree -- so all of them hold the same bits and no third launch is needed; norm =
//                           float(sqrt(sum)), coef = om_clip_coef.  Workgroup 0 writes {norm, coef} to `state`.  With `coef_in` the sum
//                           is skipped and the caller's coefficient is used.  Then optim_math.h on the workgroup's chunk.
//   prcnn_optim_step_adam,  the same prologue, then om_adam_l2 / om_sgd of optim_math.h (TRAIN.OPTIMIZER adam and sgd); a tensor without
//   prcnn_optim_step_sgd    a gradient is left alone.
// Loads and stores are 16-byte units where the chunk's four addresses (the gradient-less: its parameter's) are 16-byte aligned, and
// 4-byte units otherwise (gradient views at arbitrary offsets of a DDP bucket or of a stack's flat gradient buffer).  The gradient is
// read, never written: `.grad` keeps its unclipped values.
#include "common.h"
#include "optim_math.h"

constexpr int OPT_THREADS = 256;
constexpr int OPT_VEC_ROUNDS = 4;
constexpr int OPT_CHUNK = OPT_THREADS * 4 * OPT_VEC_ROUNDS;      // 4096 elements; PRCNN_OPTIM_CHUNK

static_assert(OPT_CHUNK == PRCNN_OPTIM_CHUNK, "include/prcnn_pointops.h and optim.hip disagree on the chunk length");
static_assert(sizeof(prcnn_optim_tensor_t) == 40 && sizeof(prcnn_optim_chunk_t) == 16, "table rows are 5 and 2 eight-byte words");

// block-wide sum in a fixed order; every lane returns the same bits.  s_red: OPT_THREADS / 64 doubles
__device__ __forceinline__ double opt_block_sum(double v, double* s_red) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s_red[0];
    for (int w = 1; w < OPT_THREADS / 64; ++w) t += s_red[w];
    return t;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_norm_kernel(const prcnn_optim_tensor_t* __restrict__ tensors,
                                                                 const prcnn_optim_chunk_t* __restrict__ chunks,
                                                                 double* __restrict__ partial) {
    __shared__ double s_red[OPT_THREADS / 64];
    const prcnn_optim_chunk_t c = chunks[blockIdx.x];
    const prcnn_optim_tensor_t T = tensors[c.tensor];
    double acc = 0.0;
    if (T.grad != nullptr) {
        const int64_t left = T.numel - c.first;
        const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
        const float* g = T.grad + c.first;
        const bool vec = ((uintptr_t)g & 15) == 0;
#pragma unroll
        for (int k = 0; k < OPT_VEC_ROUNDS; ++k) {
            const int base = (k * OPT_THREADS + (int)threadIdx.x) * 4;
            if (vec && base + 4 <= n) {
                const float4 x = *(const float4*)(g + base);
                acc += (double)x.x * (double)x.x;
                acc += (double)x.y * (double)x.y;
                acc += (double)x.z * (double)x.z;
                acc += (double)x.w * (double)x.w;
            } else {
                for (int j = base; j < base + 4 && j < n; ++j) {
                    const double x = (double)g[j];
                    acc += x * x;
                }
            }
        }
    }
    const double t = opt_block_sum(acc, s_red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// the clip coefficient of one step, the same bits in every lane of every workgroup: the caller's, or formed from the partial sums
__device__ __forceinline__ float opt_coef(int64_t num_chunks, const double* __restrict__ partial, float max_norm,
                                          const float* __restrict__ coef_in, float* __restrict__ state, double* s_red) {
    if (coef_in != nullptr) return coef_in[0];
    const int64_t per = (num_chunks + OPT_THREADS - 1) / OPT_THREADS;
    const int64_t b0 = (int64_t)threadIdx.x * per;
    const int64_t b1 = b0 + per < num_chunks ? b0 + per : num_chunks;
    double acc = 0.0;
    for (int64_t b = b0; b < b1; ++b) acc += partial[b];
    const float norm = (float)sqrt(opt_block_sum(acc, s_red));
    const float coef = om_clip_coef(norm, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        state[0] = norm;
        state[1] = coef;
    }
    return coef;
}

__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const prcnn_optim_tensor_t* __restrict__ tensors,
                                                                   const prcnn_optim_chunk_t* __restrict__ chunks, int64_t num_chunks,
                                                                   const double* __restrict__ partial, float max_norm,
                                                                   const float* __restrict__ coef_in, float* __restrict__ state,
                                                                   const OmScalars S) {
    __shared__ double s_red[OPT_THREADS / 64];
    const float coef = opt_coef(num_chunks, partial, max_norm, coef_in, state, s_red);

    const prcnn_optim_chunk_t c = chunks[blockIdx.x];
    const prcnn_optim_tensor_t T = tensors[c.tensor];
    const int64_t left = T.numel - c.first;
    const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    float* p = T.param + c.first;
    if (T.grad == nullptr) {                                  // decay only; the moments are not touched
        const bool vec = ((uintptr_t)p & 15) == 0;
#pragma unroll
        for (int k = 0; k < OPT_VEC_ROUNDS; ++k) {
            const int base = (k * OPT_THREADS + (int)threadIdx.x) * 4;
            if (vec && base + 4 <= n) {
                float4 x = *(const float4*)(p + base);
                x.x = om_decay(x.x, S);
                x.y = om_decay(x.y, S);
                x.z = om_decay(x.z, S);
                x.w = om_decay(x.w, S);
                *(float4*)(p + base) = x;
            } else {
                for (int j = base; j < base + 4 && j < n; ++j) p[j] = om_decay(p[j], S);
            }
        }
        return;
    }
    const float* g = T.grad + c.first;
    float* m = T.exp_avg + c.first;
    float* v = T.exp_avg_sq + c.first;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
#pragma unroll
    for (int k = 0; k < OPT_VEC_ROUNDS; ++k) {
        const int base = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        if (vec && base + 4 <= n) {
            float4 xp = *(const float4*)(p + base);
            const float4 xg = *(const float4*)(g + base);
            float4 xm = *(const float4*)(m + base);
            float4 xv = *(const float4*)(v + base);
            om_update(&xp.x, xg.x, &xm.x, &xv.x, coef, S);
            om_update(&xp.y, xg.y, &xm.y, &xv.y, coef, S);
            om_update(&xp.z, xg.z, &xm.z, &xv.z, coef, S);
            om_update(&xp.w, xg.w, &xm.w, &xv.w, coef, S);
            *(float4*)(p + base) = xp;
            *(float4*)(m + base) = xm;
            *(float4*)(v + base) = xv;
        } else {
            for (int j = base; j < base + 4 && j < n; ++j) {
                float xp = p[j], xm = m[j], xv = v[j];
                om_update(&xp, g[j], &xm, &xv, coef, S);
                p[j] = xp;
                m[j] = xm;
                v[j] = xv;
            }
        }
    }
}

// TRAIN.OPTIMIZER adam and sgd (optim.py ClipAdam / ClipSGD): the same tables, chunks, lanes and access rule; a tensor without a
// gradient is left alone.  adam: four streams per element; sgd: three (the momentum buffer is the row's exp_avg), two with
// momentum == 0, when exp_avg is not read and may be null.
__global__ __launch_bounds__(OPT_THREADS) void optim_adam_l2_kernel(const prcnn_optim_tensor_t* __restrict__ tensors,
                                                                    const prcnn_optim_chunk_t* __restrict__ chunks, int64_t num_chunks,
                                                                    const double* __restrict__ partial, float max_norm,
                                                                    const float* __restrict__ coef_in, float* __restrict__ state,
                                                                    const OmAdamL2 S) {
    __shared__ double s_red[OPT_THREADS / 64];
    const float coef = opt_coef(num_chunks, partial, max_norm, coef_in, state, s_red);

    const prcnn_optim_chunk_t c = chunks[blockIdx.x];
    const prcnn_optim_tensor_t T = tensors[c.tensor];
    if (T.grad == nullptr) return;
    const int64_t left = T.numel - c.first;
    const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    float* p = T.param + c.first;
    const float* g = T.grad + c.first;
    float* m = T.exp_avg + c.first;
    float* v = T.exp_avg_sq + c.first;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
#pragma unroll
    for (int k = 0; k < OPT_VEC_ROUNDS; ++k) {
        const int base = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        if (vec && base + 4 <= n) {
            float4 xp = *(const float4*)(p + base);
            const float4 xg = *(const float4*)(g + base);
            float4 xm = *(const float4*)(m + base);
            float4 xv = *(const float4*)(v + base);
            om_adam_l2(&xp.x, xg.x, &xm.x, &xv.x, coef, S);
            om_adam_l2(&xp.y, xg.y, &xm.y, &xv.y, coef, S);
            om_adam_l2(&xp.z, xg.z, &xm.z, &xv.z, coef, S);
            om_adam_l2(&xp.w, xg.w, &xm.w, &xv.w, coef, S);
            *(float4*)(p + base) = xp;
            *(float4*)(m + base) = xm;
            *(float4*)(v + base) = xv;
        } else {
            for (int j = base; j < base + 4 && j < n; ++j) {
                float xp = p[j], xm = m[j], xv = v[j];
                om_adam_l2(&xp, g[j], &xm, &xv, coef, S);
                p[j] = xp;
                m[j] = xm;
                v[j] = xv;
            }
        }
    }
}

template <bool MOMENTUM>
__global__ __launch_bounds__(OPT_THREADS) void optim_sgd_kernel(const prcnn_optim_tensor_t* __restrict__ tensors,
                                                                const prcnn_optim_chunk_t* __restrict__ chunks, int64_t num_chunks,
                                                                const double* __restrict__ partial, float max_norm,
                                                                const float* __restrict__ coef_in, float* __restrict__ state,
                                                                const OmSgd S) {
    __shared__ double s_red[OPT_THREADS / 64];
    const float coef = opt_coef(num_chunks, partial, max_norm, coef_in, state, s_red);

    const prcnn_optim_chunk_t c = chunks[blockIdx.x];
    const prcnn_optim_tensor_t T = tensors[c.tensor];
    if (T.grad == nullptr) return;
    const int64_t left = T.numel - c.first;
    const int n = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    float* p = T.param + c.first;
    const float* g = T.grad + c.first;
    float* m = MOMENTUM ? T.exp_avg + c.first : nullptr;
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) == 0;
#pragma unroll
    for (int k = 0; k < OPT_VEC_ROUNDS; ++k) {
        const int base = (k * OPT_THREADS + (int)threadIdx.x) * 4;
        if (vec && base + 4 <= n) {
            float4 xp = *(const float4*)(p + base);
            const float4 xg = *(const float4*)(g + base);
            if constexpr (MOMENTUM) {
                float4 xm = *(const float4*)(m + base);
                om_sgd(&xp.x, xg.x, &xm.x, coef, S);
                om_sgd(&xp.y, xg.y, &xm.y, coef, S);
                om_sgd(&xp.z, xg.z, &xm.z, coef, S);
                om_sgd(&xp.w, xg.w, &xm.w, coef, S);
                *(float4*)(m + base) = xm;
            } else {
                om_sgd_plain(&xp.x, xg.x, coef, S);
                om_sgd_plain(&xp.y, xg.y, coef, S);
                om_sgd_plain(&xp.z, xg.z, coef, S);
                om_sgd_plain(&xp.w, xg.w, coef, S);
            }
            *(float4*)(p + base) = xp;
        } else {
            for (int j = base; j < base + 4 && j < n; ++j) {
                float xp = p[j];
                if constexpr (MOMENTUM) {
                    float xm = m[j];
                    om_sgd(&xp, g[j], &xm, coef, S);
                    m[j] = xm;
                } else {
                    om_sgd_plain(&xp, g[j], coef, S);
                }
                p[j] = xp;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ exports
static int opt_tables(const char* who, const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks) {
    PRCNN_REQUIRE(num_chunks >= 0 && num_chunks < ((int64_t)1 << 31), "%s: bad chunk count %lld", who, (long long)num_chunks);
    if (num_chunks > 0) {
        PRCNN_REQUIRE(tensors && chunks, "%s: null table", who);
        PRCNN_REQUIRE((uintptr_t)tensors % 8 == 0 && (uintptr_t)chunks % 8 == 0, "%s: the tables must be 8-byte aligned", who);
    }
    return PRCNN_OK;
}

// the clip arguments the three update exports share
static int opt_clip_args(const char* who, int64_t num_chunks, const double* partial, float max_norm, const float* coef, float* state) {
    if (coef != nullptr) return PRCNN_OK;
    PRCNN_REQUIRE(state != nullptr, "%s: without a caller's coef the {norm, coef} state must be given", who);
    PRCNN_REQUIRE(num_chunks == 0 || (partial && (uintptr_t)partial % 8 == 0),
                  "%s: without a caller's coef the partial sums of prcnn_optim_grad_norm must be given (8-byte aligned)", who);
    PRCNN_REQUIRE(max_norm > 0.0f, "%s: max_norm must be > 0, got %g", who, (double)max_norm);
    return PRCNN_OK;
}

PRCNN_API size_t prcnn_optim_chunk_elems(void) { return (size_t)OPT_CHUNK; }

PRCNN_API int prcnn_optim_grad_norm(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks,
                                    double* partial, prcnn_stream_t stream) {
    const int rc = opt_tables("prcnn_optim_grad_norm", tensors, chunks, num_chunks);
    if (rc != PRCNN_OK) return rc;
    if (num_chunks == 0) return PRCNN_OK;
    PRCNN_REQUIRE(partial && (uintptr_t)partial % 8 == 0, "prcnn_optim_grad_norm: partial must be a non-null, 8-byte aligned pointer");
    hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)num_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks, partial);
    PRCNN_LAUNCH_CHECK("prcnn_optim_grad_norm");
    return PRCNN_OK;
}

PRCNN_API int prcnn_optim_step(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks,
                               const double* partial, float max_norm, const float* coef, float* state, float decay,
                               float one_minus_beta1, float beta2, float one_minus_beta2, float bias2_sqrt, float eps, float neg_step,
                               prcnn_stream_t stream) {
    int rc = opt_tables("prcnn_optim_step", tensors, chunks, num_chunks);
    if (rc != PRCNN_OK) return rc;
    rc = opt_clip_args("prcnn_optim_step", num_chunks, partial, max_norm, coef, state);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(bias2_sqrt > 0.0f, "prcnn_optim_step: sqrt(1 - beta2^t) must be > 0, got %g", (double)bias2_sqrt);
    if (num_chunks == 0) return PRCNN_OK;
    const OmScalars S = {decay, one_minus_beta1, beta2, one_minus_beta2, bias2_sqrt, eps, neg_step};
    hipLaunchKernelGGL(optim_update_kernel, dim3((unsigned)num_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                       num_chunks, partial, max_norm, coef, state, S);
    PRCNN_LAUNCH_CHECK("prcnn_optim_step");
    return PRCNN_OK;
}

PRCNN_API int prcnn_optim_step_adam(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks,
                                    const double* partial, float max_norm, const float* coef, float* state, float weight_decay,
                                    float one_minus_beta1, float beta2, float one_minus_beta2, float bias2_sqrt, float eps, float neg_step,
                                    prcnn_stream_t stream) {
    int rc = opt_tables("prcnn_optim_step_adam", tensors, chunks, num_chunks);
    if (rc != PRCNN_OK) return rc;
    rc = opt_clip_args("prcnn_optim_step_adam", num_chunks, partial, max_norm, coef, state);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(bias2_sqrt > 0.0f, "prcnn_optim_step_adam: sqrt(1 - beta2^t) must be > 0, got %g", (double)bias2_sqrt);
    PRCNN_REQUIRE(weight_decay >= 0.0f, "prcnn_optim_step_adam: weight_decay must be >= 0, got %g", (double)weight_decay);
    if (num_chunks == 0) return PRCNN_OK;
    const OmAdamL2 S = {weight_decay, one_minus_beta1, beta2, one_minus_beta2, bias2_sqrt, eps, neg_step};
    hipLaunchKernelGGL(optim_adam_l2_kernel, dim3((unsigned)num_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                       num_chunks, partial, max_norm, coef, state, S);
    PRCNN_LAUNCH_CHECK("prcnn_optim_step_adam");
    return PRCNN_OK;
}

PRCNN_API int prcnn_optim_step_sgd(const prcnn_optim_tensor_t* tensors, const prcnn_optim_chunk_t* chunks, int64_t num_chunks,
                                   const double* partial, float max_norm, const float* coef, float* state, float weight_decay,
                                   float momentum, float neg_lr, prcnn_stream_t stream) {
    int rc = opt_tables("prcnn_optim_step_sgd", tensors, chunks, num_chunks);
    if (rc != PRCNN_OK) return rc;
    rc = opt_clip_args("prcnn_optim_step_sgd", num_chunks, partial, max_norm, coef, state);
    if (rc != PRCNN_OK) return rc;
    PRCNN_REQUIRE(weight_decay >= 0.0f, "prcnn_optim_step_sgd: weight_decay must be >= 0, got %g", (double)weight_decay);
    PRCNN_REQUIRE(momentum >= 0.0f, "prcnn_optim_step_sgd: momentum must be >= 0, got %g", (double)momentum);
    if (num_chunks == 0) return PRCNN_OK;
    const OmSgd S = {weight_decay, momentum, neg_lr};
    if (momentum != 0.0f)
        hipLaunchKernelGGL(optim_sgd_kernel<true>, dim3((unsigned)num_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                           num_chunks, partial, max_norm, coef, state, S);
    else
        hipLaunchKernelGGL(optim_sgd_kernel<false>, dim3((unsigned)num_chunks), dim3(OPT_THREADS), 0, (hipStream_t)stream, tensors, chunks,
                           num_chunks, partial, max_norm, coef, state, S);
    PRCNN_LAUNCH_CHECK("prcnn_optim_step_sgd");
    return PRCNN_OK;
}
