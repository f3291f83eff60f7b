// head_tail.hip -- the tail of a training head on channels-last rows: Dropout keyed by a counter (head_tail_math.h) and the output
// layer, forward and backward, fp32 MFMA (v_mfma_f32_32x32x2_f32).  No mask and no dropped copy of x exist in memory: forward
// applies the mask while it loads a row, backward rebuilds it from the same key.
//   prcnn_head_tail_fwd    out[r, n] = sum_k drop(x)[r, k] w[n, k] + b[n]
//   prcnn_head_tail_bwd    one pass over x and g: gx[r, k] = keep ? scale * sum_n g[r, n] w[n, k] : 0, and per-workgroup partial
//                          tiles of gw[n, k] = sum_r g[r, n] drop(x)[r, k] and gb[n] = sum_r g[r, n]; a second launch adds the
//                          partials in a fixed order.  No atomics, no memset: the same state gives the same bytes.
//   prcnn_dropout_rows     out = drop(x) (a Dropout that no output layer follows; backward is the same call on the gradient)
// MFMA operand layout (one float per lane and operand, lane = (h = lane >> 5, j = lane & 31)): A[row j][k = h], B[k = h][col j];
// C[row (e & 3) + 8 (e >> 2) + 4 h][col j] in element e of the 16 accumulator registers -- as train_wgrad_kernel (mlp_train.h).
// Which two of the summed index's values a step takes is free as long as A and B agree; the order is fixed by the shape alone
// (K and N), never by R: a row's output bits depend on its own row, its index r and the weights only.
//
// Forward: a wave owns 32 rows and all N outputs (NB = ceil(N / 32) accumulator blocks).  Lane (h, j) loads 16 bytes of row j per
// step (channels 8 s + 4 h ..), masks them and feeds four MFMA steps; the weights sit in LDS, row stride K + 4 floats, so that the
// 32 lanes' ds_read_b128 of 32 different weight rows fall on different banks.  A workgroup stages the weights once and walks row
// tiles in a grid-stride loop.
// Backward: a workgroup owns HT_BWD_ROWS consecutive rows = one partial tile, staged HT_CHUNK rows at a time into LDS (16-byte global
// loads of x, the mask applied on the way; g element-wise, since its rows arrive as views with any stride), the next chunk's loads in
// flight in registers while the current one is multiplied.  The four waves split K's 32-channel blocks (wave, wave + 4): for its
// blocks a wave computes gx (sum over n, g as A, w as B) and accumulates gw (sum over the rows, drop(x) as A, g as B).  Row strides
// in LDS: K or K + 32 floats (= 32 mod 64 banks: the two halves of a wave read two consecutive rows; plain K where that lets two
// workgroups share a CU), N rounded up to 32 plus 2 for g.
#include "common.h"
#include "head_tail_math.h"

typedef float ht_f32x16 __attribute__((ext_vector_type(16)));

constexpr int HT_THREADS = 256;
constexpr int HT_FWD_ROWS = 128;         // 4 waves x 32 rows
constexpr int HT_FWD_GRID = 1024;
constexpr int HT_CHUNK = 32;             // rows staged per step of the backward
constexpr int HT_BWD_ROWS = 512;         // rows per workgroup of the backward = rows per partial tile (ops.HEAD_TAIL_PART_ROWS)
constexpr int HT_LDS_MAX = 160 * 1024;

struct HtKey {
    unsigned key;        // head_tail_key(seed, stream, call)
    float p, scale;
};

__device__ __forceinline__ int ht_c_row(int e, int h) { return (e & 3) + 8 * (e >> 2) + 4 * h; }

template <int NB>
__global__ __launch_bounds__(HT_THREADS) void head_tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ b, float* __restrict__ out, long R, int K,
                                                                   int N, HtKey M, long tiles) {
    extern __shared__ __attribute__((aligned(16))) float ht_lds[];
    const int WS = K + 4, kq = K / 4;
    for (int idx = threadIdx.x; idx < NB * 32 * kq; idx += HT_THREADS) {
        const int n = idx / kq, c = idx - n * kq;
        const float4 v = n < N ? *reinterpret_cast<const float4*>(w + (long)n * K + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(ht_lds + n * WS + 4 * c) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = lane >> 5, j = lane & 31;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long r0 = tile * HT_FWD_ROWS + wave * 32;
        if (r0 >= R) continue;
        const long r = r0 + j < R ? r0 + j : R - 1;            // rows past the end: a valid row is read, nothing is stored
        const float* xr = x + r * K + 4 * h;
        const unsigned i0 = (unsigned)((unsigned long long)r * (unsigned)K) + 4 * h;
        const float* wl = ht_lds + j * WS + 4 * h;
        ht_f32x16 acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; nb++) acc[nb] = (ht_f32x16){0};
        // four steps (32 channels) at a time, their global loads issued together ahead of the MFMA work (K is a multiple of 32)
        for (int s0 = 0; s0 < K / 8; s0 += 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const float4*>(xr + 8 * (s0 + u));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int s = s0 + u;
                const float xv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                float a[4];
#pragma unroll
                for (int e = 0; e < 4; e++) a[e] = head_tail_drop(xv[e], head_tail_keep_i(M.key, i0 + 8 * s + e, M.p), M.scale);
                float4 wv[NB];
#pragma unroll
                for (int nb = 0; nb < NB; nb++) wv[nb] = *reinterpret_cast<const float4*>(wl + nb * 32 * WS + 8 * s);
#pragma unroll
                for (int nb = 0; nb < NB; nb++) {
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], wv[nb].x, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], wv[nb].y, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], wv[nb].z, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], wv[nb].w, acc[nb], 0, 0, 0);
                }
            }
        }
        // C[row][col j]: row r0 + ht_c_row(e, h), output channel nb * 32 + j
#pragma unroll
        for (int nb = 0; nb < NB; nb++) {
            const int n = nb * 32 + j;
            if (n >= N) continue;
            const float bias = b ? b[n] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const long rr = r0 + ht_c_row(e, h);
                if (rr < R) out[rr * N + n] = b ? acc[nb][e] + bias : acc[nb][e];
            }
        }
    }
}

struct HtBwd {
    const float* x;          // (R, K); read only when gw is wanted
    const float* w;          // (N, K); read only when gx is wanted
    const float* g;          // (R, N), row stride ldg
    long ldg;
    float* gx;               // (R, K) | null
    float* part;             // (parts, N * K + N): the partial gw tile, then the partial gb | null when neither is wanted
    long R;
    int K, N;
    int KS;                  // row stride of the w and drop(x) tiles in LDS, floats (ht_launch_bwd)
    int want_gw, want_gb;
    HtKey M;
};

// KB2: 32-channel blocks of K per wave (K <= 128: 1, else 2); NB: 32-channel blocks of N
template <int KB2, int NB>
__global__ __launch_bounds__(HT_THREADS) void head_tail_bwd_kernel(const HtBwd P) {
    extern __shared__ __attribute__((aligned(16))) float ht_lds[];
    constexpr int NP = NB * 32, GS = NP + 2;
    const int K = P.K, N = P.N, kq = K / 4, kblocks = K / 32;
    const long R = P.R;
    const int KS = P.KS;
    const bool want_gx = P.gx != nullptr, want_gw = P.want_gw != 0, want_gb = P.want_gb != 0;
    float* wL = ht_lds;                                  // NP x KS, rows past N zero (only with gx)
    float* xL = wL + (want_gx ? NP * KS : 0);            // HT_CHUNK x KS: drop(x)
    float* gL = xL + (want_gw ? HT_CHUNK * KS : 0);      // HT_CHUNK x GS, columns past N zero
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, j = lane & 31;
    if (want_gx)
        for (int idx = tid; idx < NP * kq; idx += HT_THREADS) {
            const int n = idx / kq, c = idx - n * kq;
            const float4 v = n < N ? *reinterpret_cast<const float4*>(P.w + (long)n * K + 4 * c) : make_float4(0.f, 0.f, 0.f, 0.f);
            *reinterpret_cast<float4*>(wL + n * KS + 4 * c) = v;
        }
    const long base = (long)blockIdx.x * HT_BWD_ROWS;
    const long left = R - base < HT_BWD_ROWS ? R - base : HT_BWD_ROWS;
    const int chunks = (int)((left + HT_CHUNK - 1) / HT_CHUNK);

    float4 xr[KB2 * 4];
    float gr[NB * 4];
    auto load = [&](long rb) {
        if (want_gw) {
#pragma unroll
            for (int i = 0; i < KB2 * 4; i++) {
                xr[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < kblocks) {
                    const int idx = i * HT_THREADS + tid;
                    const int row = idx / kq, c = idx - row * kq;
                    if (rb + row < R) xr[i] = *reinterpret_cast<const float4*>(P.x + (rb + row) * K + 4 * c);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NB * 4; i++) {
            const int idx = i * HT_THREADS + tid;
            const int row = idx / NP, n = idx - row * NP;
            gr[i] = (rb + row < R && n < N) ? P.g[(rb + row) * P.ldg + n] : 0.f;
        }
    };
    auto stage = [&](long rb) {
        if (want_gw) {
#pragma unroll
            for (int i = 0; i < KB2 * 4; i++) {
                if (i < kblocks) {
                    const int idx = i * HT_THREADS + tid;
                    const int row = idx / kq, c = idx - row * kq;
                    const unsigned i0 = (unsigned)((unsigned long long)(rb + row) * (unsigned)K) + 4 * c;
                    float4 v;
                    v.x = head_tail_drop(xr[i].x, head_tail_keep_i(P.M.key, i0, P.M.p), P.M.scale);
                    v.y = head_tail_drop(xr[i].y, head_tail_keep_i(P.M.key, i0 + 1, P.M.p), P.M.scale);
                    v.z = head_tail_drop(xr[i].z, head_tail_keep_i(P.M.key, i0 + 2, P.M.p), P.M.scale);
                    v.w = head_tail_drop(xr[i].w, head_tail_keep_i(P.M.key, i0 + 3, P.M.p), P.M.scale);
                    *reinterpret_cast<float4*>(xL + row * KS + 4 * c) = v;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NB * 4; i++) {
            const int idx = i * HT_THREADS + tid;
            const int row = idx / NP, n = idx - row * NP;
            gL[row * GS + n] = gr[i];
        }
    };

    ht_f32x16 accw[KB2][NB];
#pragma unroll
    for (int q = 0; q < KB2; q++)
#pragma unroll
        for (int nb = 0; nb < NB; nb++) accw[q][nb] = (ht_f32x16){0};
    float gbacc = 0.f;

    load(base);
    for (int c = 0; c < chunks; c++) {
        const long rb = base + (long)c * HT_CHUNK;
        stage(rb);
        __syncthreads();
        if (c + 1 < chunks) load(rb + HT_CHUNK);
        if (want_gb && tid < NP) {
#pragma unroll 8
            for (int row = 0; row < HT_CHUNK; row++) gbacc += gL[row * GS + tid];
        }
#pragma unroll
        for (int q = 0; q < KB2; q++) {
            const int cb = wave + 4 * q;
            if (cb >= kblocks) continue;
            if (want_gx) {
                // C[row][col j] = sum_n g[row][n] w[n][cb * 32 + j]
                ht_f32x16 acc = (ht_f32x16){0};
                const float* ga = gL + j * GS + h;
                const float* wb = wL + h * KS + cb * 32 + j;
#pragma unroll 8
                for (int t = 0; t < NP / 2; t++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * t], wb[2 * t * KS], acc, 0, 0, 0);
                const int k = cb * 32 + j;
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const long rr = rb + ht_c_row(e, h);
                    if (rr < R) {
                        const unsigned i = (unsigned)((unsigned long long)rr * (unsigned)K) + k;
                        P.gx[rr * K + k] = head_tail_keep_i(P.M.key, i, P.M.p) ? acc[e] * P.M.scale : 0.f;
                    }
                }
            }
            if (want_gw) {
                // C[channel i][col j] += sum_rows drop(x)[row][cb * 32 + i] g[row][nb * 32 + j]
                const float* xa = xL + h * KS + cb * 32 + j;
                const float* gb = gL + h * GS + j;
#pragma unroll 4
                for (int t = 0; t < HT_CHUNK / 2; t++) {
                    const float a = xa[2 * t * KS];
#pragma unroll
                    for (int nb = 0; nb < NB; nb++)
                        accw[q][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, gb[2 * t * GS + nb * 32], accw[q][nb], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }
    if (!want_gw && !want_gb) return;
    float* part = P.part + (long)blockIdx.x * ((long)N * K + N);
    if (want_gw) {
#pragma unroll
        for (int q = 0; q < KB2; q++) {
            const int cb = wave + 4 * q;
            if (cb >= kblocks) continue;
#pragma unroll
            for (int nb = 0; nb < NB; nb++) {
                const int n = nb * 32 + j;
                if (n >= N) continue;
#pragma unroll
                for (int e = 0; e < 16; e++) part[(long)n * K + cb * 32 + ht_c_row(e, h)] = accw[q][nb][e];
            }
        }
    }
    if (want_gb && tid < N) part[(long)N * K + tid] = gbacc;
}

// gw[e] (e < N K) and gb[e - N K]: the partial tiles added in a fixed order.  Block = HT_RED_E elements x HT_RED_Q lanes over the partial
// index (as train_wgrad_reduce_kernel, mlp_train.h): lane q adds its contiguous range of partials, four loads in flight, and lane 0 of
// an element adds the HT_RED_Q sums in order.
constexpr int HT_RED_E = 16, HT_RED_Q = 16;
__global__ __launch_bounds__(HT_THREADS) void head_tail_reduce_kernel(const float* __restrict__ part, int parts, int NK, int N,
                                                                      float* __restrict__ gw, float* __restrict__ gb) {
    __shared__ float sm[HT_RED_Q][HT_RED_E];
    const int c = threadIdx.x & (HT_RED_E - 1), q = threadIdx.x / HT_RED_E;
    const int e = blockIdx.x * HT_RED_E + c;
    const bool live = e < NK + N;
    const long stride = (long)NK + N;
    float s = 0.f;
    if (live) {
        const int per = (parts + HT_RED_Q - 1) / HT_RED_Q;
        const int p1 = min(parts, (q + 1) * per);
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int p = q * per;
        for (; p + 4 <= p1; p += 4) {
            a0 += part[(long)p * stride + e];
            a1 += part[(long)(p + 1) * stride + e];
            a2 += part[(long)(p + 2) * stride + e];
            a3 += part[(long)(p + 3) * stride + e];
        }
        for (; p < p1; p++) a0 += part[(long)p * stride + e];
        s = (a0 + a1) + (a2 + a3);
    }
    sm[q][c] = s;
    __syncthreads();
    if (q != 0 || !live) return;
    float* dst = e < NK ? (gw ? gw + e : nullptr) : (gb ? gb + (e - NK) : nullptr);
    if (!dst) return;
    float tot = 0.f;
#pragma unroll
    for (int u = 0; u < HT_RED_Q; u++) tot += sm[u][c];
    *dst = tot;
}

__global__ __launch_bounds__(HT_THREADS) void dropout_rows_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                  unsigned long long quads, HtKey M) {
    for (unsigned long long q = (unsigned long long)blockIdx.x * HT_THREADS + threadIdx.x; q < quads;
         q += (unsigned long long)gridDim.x * HT_THREADS) {
        const float4 v = reinterpret_cast<const float4*>(x)[q];
        const unsigned i0 = (unsigned)(q * 4);
        float4 o;
        o.x = head_tail_drop(v.x, head_tail_keep_i(M.key, i0, M.p), M.scale);
        o.y = head_tail_drop(v.y, head_tail_keep_i(M.key, i0 + 1, M.p), M.scale);
        o.z = head_tail_drop(v.z, head_tail_keep_i(M.key, i0 + 2, M.p), M.scale);
        o.w = head_tail_drop(v.w, head_tail_keep_i(M.key, i0 + 3, M.p), M.scale);
        reinterpret_cast<float4*>(out)[q] = o;
    }
}

// ---- C ABI ---------------------------------------------------------------------------------------------------------------------
static bool ht_domain(int64_t R, int K, int N) {
    return R >= 1 && K >= 32 && K <= 256 && K % 32 == 0 && N >= 1 && N <= 96 && (unsigned long long)R * (unsigned)K <= (1ull << 32);
}
static bool ht_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static HtKey ht_key(uint32_t seed, uint32_t stream, uint32_t call, float p) {
    return HtKey{head_tail_key(seed, stream, call), p, head_tail_scale(p)};
}
static long ht_parts(int64_t R) { return (long)((R + HT_BWD_ROWS - 1) / HT_BWD_ROWS); }

template <int NB>
static int ht_launch_fwd(const float* x, const float* w, const float* b, float* out, int64_t R, int K, int N, HtKey M, hipStream_t s) {
    static PrcnnLdsLimit lim;
    const int lds = NB * 32 * (K + 4) * (int)sizeof(float);
    if (lds > 64 * 1024 && !lim.raise((const void*)head_tail_fwd_kernel<NB>, HT_LDS_MAX))
        return prcnn_fail(PRCNN_EHIP, "prcnn_head_tail_fwd: cannot raise the dynamic LDS limit");
    const long tiles = (R + HT_FWD_ROWS - 1) / HT_FWD_ROWS;
    const unsigned grid = (unsigned)(tiles < HT_FWD_GRID ? tiles : HT_FWD_GRID);
    hipLaunchKernelGGL(head_tail_fwd_kernel<NB>, dim3(grid), dim3(HT_THREADS), lds, s, x, w, b, out, (long)R, K, N, M, tiles);
    PRCNN_LAUNCH_CHECK("prcnn_head_tail_fwd");
    return PRCNN_OK;
}

template <int KB2, int NB>
static int ht_launch_bwd(HtBwd& P, hipStream_t s) {
    static PrcnnLdsLimit lim;
    auto lds_bytes = [&](int ks) {
        return ((P.gx ? NB * 32 * ks : 0) + (P.want_gw ? HT_CHUNK * ks : 0) + HT_CHUNK * (NB * 32 + 2)) * (int)sizeof(float);
    };
    // the padded stride keeps the two halves of a wave on different banks; where dropping it lets a second workgroup share the CU
    // (its staging and barriers then run under the other's MFMA work), that is worth more than the two-way conflict it brings back
    P.KS = (P.K % 64 == 0) ? P.K + 32 : P.K;
    if (lds_bytes(P.KS) > HT_LDS_MAX / 2 && lds_bytes(P.K) <= HT_LDS_MAX / 2) P.KS = P.K;
    const int lds = lds_bytes(P.KS);
    if (lds > HT_LDS_MAX) return prcnn_fail(PRCNN_EUNSUPPORTED, "prcnn_head_tail_bwd: %d bytes of LDS", lds);
    if (lds > 64 * 1024 && !lim.raise((const void*)head_tail_bwd_kernel<KB2, NB>, HT_LDS_MAX))
        return prcnn_fail(PRCNN_EHIP, "prcnn_head_tail_bwd: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL((head_tail_bwd_kernel<KB2, NB>), dim3((unsigned)ht_parts(P.R)), dim3(HT_THREADS), lds, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_head_tail_bwd");
    return PRCNN_OK;
}

PRCNN_API int prcnn_head_tail_fwd(const float* x, const float* w, const float* b, float* out, int64_t R, int K, int N, uint32_t seed,
                                  uint32_t stream_id, uint32_t call, float p, prcnn_stream_t stream) {
    PRCNN_REQUIRE(ht_domain(R, K, N), "prcnn_head_tail_fwd: (R, K, N) = (%lld, %d, %d) outside the domain", (long long)R, K, N);
    PRCNN_REQUIRE(p >= 0.0f && p < 1.0f, "prcnn_head_tail_fwd: p must lie in [0, 1), got %g", (double)p);
    PRCNN_REQUIRE(x && w && out, "prcnn_head_tail_fwd: null pointer");
    PRCNN_REQUIRE(ht_aligned16(x) && ht_aligned16(w), "prcnn_head_tail_fwd: x and w must be 16-byte aligned");
    const HtKey M = ht_key(seed, stream_id, call, p);
    const int nb = (N + 31) / 32;
    hipStream_t s = (hipStream_t)stream;
    if (nb == 1) return ht_launch_fwd<1>(x, w, b, out, R, K, N, M, s);
    if (nb == 2) return ht_launch_fwd<2>(x, w, b, out, R, K, N, M, s);
    return ht_launch_fwd<3>(x, w, b, out, R, K, N, M, s);
}

PRCNN_API size_t prcnn_head_tail_work_bytes(int64_t R, int K, int N) {
    if (!ht_domain(R, K, N)) return 0;
    return (size_t)ht_parts(R) * ((size_t)N * K + N) * sizeof(float);
}

PRCNN_API int prcnn_head_tail_bwd(const float* x, const float* w, const float* g, int64_t ldg, float* gx, float* gw, float* gb, void* work,
                                  size_t work_bytes, int64_t R, int K, int N, uint32_t seed, uint32_t stream_id, uint32_t call, float p,
                                  prcnn_stream_t stream) {
    PRCNN_REQUIRE(ht_domain(R, K, N), "prcnn_head_tail_bwd: (R, K, N) = (%lld, %d, %d) outside the domain", (long long)R, K, N);
    PRCNN_REQUIRE(p >= 0.0f && p < 1.0f, "prcnn_head_tail_bwd: p must lie in [0, 1), got %g", (double)p);
    PRCNN_REQUIRE(g && ldg >= N, "prcnn_head_tail_bwd: g null or ldg %lld < N %d", (long long)ldg, N);
    if (!gx && !gw && !gb) return PRCNN_OK;
    PRCNN_REQUIRE(!gx || (w && ht_aligned16(w)), "prcnn_head_tail_bwd: gx needs w, 16-byte aligned");
    PRCNN_REQUIRE(!gw || (x && ht_aligned16(x)), "prcnn_head_tail_bwd: gw needs x, 16-byte aligned");
    PRCNN_REQUIRE((!gw && !gb) || (work && work_bytes >= prcnn_head_tail_work_bytes(R, K, N)),
                  "prcnn_head_tail_bwd: gw / gb need a workspace of prcnn_head_tail_work_bytes(R, K, N) bytes");
    HtBwd P;
    P.x = x; P.w = w; P.g = g; P.ldg = (long)ldg; P.gx = gx; P.part = (gw || gb) ? (float*)work : nullptr;
    P.R = (long)R; P.K = K; P.N = N; P.want_gw = gw != nullptr; P.want_gb = gb != nullptr;
    P.M = ht_key(seed, stream_id, call, p);
    hipStream_t s = (hipStream_t)stream;
    const int nb = (N + 31) / 32, kb2 = K > 128 ? 2 : 1;
    int rc;
    if (kb2 == 1 && nb == 1) rc = ht_launch_bwd<1, 1>(P, s);
    else if (kb2 == 1 && nb == 2) rc = ht_launch_bwd<1, 2>(P, s);
    else if (kb2 == 1) rc = ht_launch_bwd<1, 3>(P, s);
    else if (nb == 1) rc = ht_launch_bwd<2, 1>(P, s);
    else if (nb == 2) rc = ht_launch_bwd<2, 2>(P, s);
    else rc = ht_launch_bwd<2, 3>(P, s);
    if (rc != PRCNN_OK) return rc;
    if (gw || gb) {
        const int NK = N * K;
        hipLaunchKernelGGL(head_tail_reduce_kernel, dim3((unsigned)prcnn_divup(NK + N, HT_RED_E)), dim3(HT_THREADS), 0, s, P.part,
                           (int)ht_parts(R), NK, N, gw, gb);
        PRCNN_LAUNCH_CHECK("prcnn_head_tail_bwd");
    }
    return PRCNN_OK;
}

PRCNN_API int prcnn_dropout_rows(const float* x, float* out, int64_t R, int K, uint32_t seed, uint32_t stream_id, uint32_t call, float p,
                                 prcnn_stream_t stream) {
    PRCNN_REQUIRE(R >= 1 && K >= 4 && K % 4 == 0 && (unsigned long long)R * (unsigned)K <= (1ull << 32),
                  "prcnn_dropout_rows: (R, K) = (%lld, %d) outside the domain", (long long)R, K);
    PRCNN_REQUIRE(p >= 0.0f && p < 1.0f, "prcnn_dropout_rows: p must lie in [0, 1), got %g", (double)p);
    PRCNN_REQUIRE(x && out && ht_aligned16(x) && ht_aligned16(out), "prcnn_dropout_rows: x and out must be non-null and 16-byte aligned");
    const unsigned long long quads = (unsigned long long)R * (unsigned)K / 4;
    const unsigned long long blocks = (quads + HT_THREADS - 1) / HT_THREADS;
    hipLaunchKernelGGL(dropout_rows_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(HT_THREADS), 0, (hipStream_t)stream, x, out,
                       quads, ht_key(seed, stream_id, call, p));
    PRCNN_LAUNCH_CHECK("prcnn_dropout_rows");
    return PRCNN_OK;
}
