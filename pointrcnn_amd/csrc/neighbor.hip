// neighbor.hip -- ball_query (one or two radii per scan) and three_nn for gfx950.
//
// Replaces pointnet2_cuda.ball_query_wrapper / three_nn_wrapper [UPSTREAM, not in tree]; semantics per
// SURVEY Appendix A.3 / A.5 and oracle prcnn_cpu_ball_query / prcnn_cpu_three_nn.
//
// Both are brute-force scans (compulsory HBM traffic is tiny: N*12 B per frame; the work is VALU):
// a workgroup owns 64 (ball query) or 256 (three_nn) lanes of one frame and streams the frame's candidate
// points through LDS in coalesced chunks, expanded to float4 so that the inner loop is ONE
// ds_read_b128 broadcast (all lanes read the same address: conflict-free) per candidate.  Scanning
// candidates in ascending index order makes the "first nsample hits in index order" contract fall
// out by construction -- no sort, no compaction pass.  The MSG levels query two radii around the
// same centroids: ball_query2 evaluates both in the same pass (half the scans).
//
// These entry points serve the frames below the grid thresholds of ops.py: at most 2 047 points, usually far fewer (SA3 / SA4,
// FP2 / FP3, the RCNN stage's 512-point RoI clouds).  Two things follow:
//   * a scan stages and walks the candidates a chunk HOLDS, rounded up to its step, not the chunk's 1 024 slots: a 64-point
//     level used to evaluate 16x the candidates it has;
//   * a launch with fewer than 65 536 queries cannot give the chip's 1 024 SIMDs a wave each with one lane per query, and that
//     lane walks a serial chain (ball query: one dependent store per hit).  There L = 8 .. 64 lanes share a query
//     (lanes_per_query): three_nn_kernel<L> merges the lanes' top 3 by three lexicographic minima, ball_query_lanes_kernel<L>
//     places the hits of contiguous index segments by a prefix over the lanes.  Launches that fill the chip keep one lane per
//     query (ball_query_kernel, three_nn_kernel<1>).
#include "grid_layout.h"

#define NN_THREADS 256      // three_nn has n >= 4x more query points: 256-thread blocks share each staged chunk
// BQ_THREADS, NB_CHUNK, the pair records and the scan of one ball-query block: grid_layout.h (grid.hip runs the same scan
// on the frames its grid flags as dense)

template <bool DUAL>
__global__ __launch_bounds__(BQ_THREADS) void ball_query_kernel(const float* __restrict__ xyz,
                                                                const float* __restrict__ new_xyz, int N, int M,
                                                                float r2a, int nsa, int32_t* __restrict__ idxa,
                                                                float r2b, int nsb, int32_t* __restrict__ idxb) {
    __shared__ __attribute__((aligned(16))) float spts[NB_CHUNK * 4];
    ball_query_scan_block<DUAL>(spts, xyz, new_xyz, N, M, blockIdx.y, blockIdx.x, r2a, nsa, idxa, r2b, nsb, idxb);
}

// L lanes (8 .. 64) share one centroid: the short levels have too few centroids to occupy the chip one per lane, and a lane
// that owns a whole ball writes its hits one dependent store after the other.  The frame streams through LDS in chunks of
// L << seg_log2 candidates (seg = 8 .. 64 per lane, at most NB_CHUNK per chunk); lane l tests the CONTIGUOUS segment l of the
// chunk, so lane order is index order.  Per chunk: every lane collects the hits of its segment per radius in a 64-bit mask, an
// exclusive prefix of the hit counts over the L lanes (continued from the chunks before) is the lane's write offset, and the
// lane writes its hits in index order while the offset is below nsample.  That is "the first nsample hits in index order" by
// construction; the hit written at offset 0 is the padding value (0 if there is none), padded cooperatively at the end.
// Segment l starts at pair record l * (seg / 2 + 1): one record of padding per segment, so that the lanes of a group read
// records an odd multiple of 32 bytes apart, not the same banks.
template <bool DUAL, int L>
__global__ __launch_bounds__(BQ_THREADS) void ball_query_lanes_kernel(const float* __restrict__ xyz,
                                                                      const float* __restrict__ new_xyz, int N, int M, int seg_log2,
                                                                      float r2a, int nsa, int32_t* __restrict__ idxa,
                                                                      float r2b, int nsb, int32_t* __restrict__ idxb) {
    __shared__ __attribute__((aligned(16))) float spts[(NB_CHUNK / 2 + L) * 8];
    const int b = blockIdx.y, tid = threadIdx.x, l = tid & (L - 1);
    const int m = blockIdx.x * (BQ_THREADS / L) + tid / L;
    const bool valid = m < M;
    const int seg = 1 << seg_log2, chunk = seg * L;
    const float* __restrict__ p = xyz + (size_t)b * N * 3;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) {
        const float* q = new_xyz + ((size_t)b * M + m) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    int32_t* oa = idxa + ((size_t)b * M + (valid ? m : 0)) * nsa;
    int32_t* ob = DUAL ? idxb + ((size_t)b * M + (valid ? m : 0)) * nsb : nullptr;
    int basea = 0, baseb = 0, firsta = 0, firstb = 0;          // hits of the chunks so far (the same in every lane of a group)
    const float r2max = DUAL ? fmaxf(r2a, r2b) : r2a;
    bool done = !valid;                                        // uniform over the group

    constexpr int PER_LANE = NB_CHUNK * 3 / BQ_THREADS;       // as the one-lane scan: the next chunk waits in registers
    float pre[PER_LANE];
    auto fetch_chunk = [&](int c0) {
        const int cnt = min(chunk, N - c0), cnt3 = cnt * 3, len3 = ((cnt + 7) & ~7) * 3;
        const float* src = p + (size_t)c0 * 3;
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int i = tid + u * BQ_THREADS;
            if (u * BQ_THREADS < len3) pre[u] = i < cnt3 ? src[i] : INFINITY;          // up to the 8-candidate step: +inf, never a hit
        }
    };
    fetch_chunk(0);
    for (int c0 = 0; c0 < N; c0 += chunk) {
        if (__all(done)) break;                    // single-wave workgroup: the whole block is finished
        const int len = (min(chunk, N - c0) + 7) & ~7;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int i = tid + u * BQ_THREADS;
            int pt = i / 3, c = i - pt * 3, pr = pt >> 1;
            if (i < len * 3) spts[(pr + (pr >> (seg_log2 - 1))) * 8 + c * 2 + (pt & 1)] = pre[u];
        }
        __syncthreads();
        if (c0 + chunk < N) fetch_chunk(c0 + chunk);
        unsigned long long ma = 0, mb = 0;         // bit j: candidate c0 + l * seg + j is inside ball a / b
        if (!done) {
            const float* rec = spts + l * ((seg >> 1) + 1) * 8;
            for (int i0 = 0; i0 < seg && l * seg + i0 < len; i0 += 8) {
                f32x2 d2[4];
                bool any = false;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    d2[u] = pair_sqdist(rec + (i0 / 2 + u) * 8, qx2, qy2, qz2);
                    any |= (d2[u].x < r2max) | (d2[u].y < r2max);
                }
                if (any) {
                    unsigned ha = 0, hb = 0;
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        float d = (u & 1) ? d2[u >> 1].y : d2[u >> 1].x;
                        ha |= (unsigned)(d < r2a) << u;
                        if (DUAL) hb |= (unsigned)(d < r2b) << u;
                    }
                    ma |= (unsigned long long)ha << i0;
                    mb |= (unsigned long long)hb << i0;
                }
            }
        }
        // every lane of the wave takes part in the prefix (a finished group contributes empty masks)
        const int ca = __popcll(ma), cb = __popcll(mb);
        int inca = ca, incb = cb;
#pragma unroll
        for (int d = 1; d < L; d <<= 1) {
            const int ua = __shfl_up(inca, d, L), ub = DUAL ? __shfl_up(incb, d, L) : 0;
            if (l >= d) { inca += ua; incb += ub; }
        }
        int offa = basea + inca - ca, offb = baseb + incb - cb;
        basea += __shfl(inca, L - 1, L);
        if (DUAL) baseb += __shfl(incb, L - 1, L);
        const int k0 = c0 + l * seg;
        while (ma && offa < nsa) {
            const int k = k0 + __ffsll(ma) - 1;
            ma &= ma - 1;
            if (offa == 0) firsta = k;
            oa[offa++] = k;
        }
        while (DUAL && mb && offb < nsb) {
            const int k = k0 + __ffsll(mb) - 1;
            mb &= mb - 1;
            if (offb == 0) firstb = k;
            ob[offb++] = k;
        }
        done = !valid || (basea >= nsa && (!DUAL || baseb >= nsb));
    }
    // the lane that wrote offset 0 holds the first hit, every other lane 0
#pragma unroll
    for (int s = 1; s < L; s <<= 1) {
        firsta |= __shfl_xor(firsta, s, 64);
        if (DUAL) firstb |= __shfl_xor(firstb, s, 64);
    }
    if (valid) {
        for (int s = min(basea, nsa) + l; s < nsa; s += L) oa[s] = firsta;      // pad with the first hit (0 if none)
        if (DUAL)
            for (int s = min(baseb, nsb) + l; s < nsb; s += L) ob[s] = firstb;
    }
}


// L lanes share one query (L = 1: the plain scan, one lane per query).  Lane l of a query's group takes pair records
// l, l + L, l + 2L, ... of every chunk, in ascending index order, and keeps the top 3 of ITS candidates under the strict-'<'
// insertion rule.  That rule is "the three smallest (distance, index) pairs, lexicographically, among the candidates whose
// distance compares below +inf" (grid.hip relies on the same restatement), so the group's result is three group-wide
// lexicographic minima over the lanes' heads, the winner popping its head each time; a +inf or NaN distance is never
// inserted anywhere, so what remains is (+inf, 0) as in the one-lane scan.
template <int L>
__global__ __launch_bounds__(NN_THREADS) void three_nn_kernel(const float* __restrict__ unknown,
                                                              const float* __restrict__ known, int n, int m,
                                                              float* __restrict__ dist2, int32_t* __restrict__ idx,
                                                              float* __restrict__ weight) {
    __shared__ __attribute__((aligned(16))) float spts[NB_CHUNK * 4];
    const int b = blockIdx.y, tid = threadIdx.x, l = tid & (L - 1);
    const int i = blockIdx.x * (NN_THREADS / L) + tid / L;
    const bool valid = i < n;
    const float* __restrict__ p = known + (size_t)b * m * 3;
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (valid) {
        const float* u = unknown + ((size_t)b * n + i) * 3;
        ux = u[0]; uy = u[1]; uz = u[2];
    }
    const f32x2 ux2 = {ux, ux}, uy2 = {uy, uy}, uz2 = {uz, uz};
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int i1 = 0, i2 = 0, i3 = 0;
    // next chunk prefetched into registers while the current one is scanned (hides the staging latency)
    constexpr int PER_LANE = NB_CHUNK * 3 / NN_THREADS;       // 12 floats of the flat xyz stream per lane per chunk
    float pre[PER_LANE];
    auto fetch_chunk = [&](int c0) {
        const int cnt3 = min(NB_CHUNK, m - c0) * 3, len3 = chunk_scan_len(m, c0, 8 * L) * 3;
        const float* src = p + (size_t)c0 * 3;
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int e = tid + u * NN_THREADS;
            if (u * NN_THREADS < len3) pre[u] = e < cnt3 ? src[e] : INFINITY;          // slots past the end: +inf, never < b3
        }
    };
    fetch_chunk(0);
    for (int c0 = 0; c0 < m; c0 += NB_CHUNK) {
        const int len = chunk_scan_len(m, c0, 8 * L);          // staged and scanned: the chunk's candidates, not its capacity
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int e = tid + u * NN_THREADS;
            int pt = e / 3, c = e - pt * 3;
            if (e < len * 3) spts[(pt >> 1) * 8 + c * 2 + (pt & 1)] = pre[u];
        }
        __syncthreads();
        if (c0 + NB_CHUNK < m) fetch_chunk(c0 + NB_CHUNK);
        for (int p0 = l; p0 < (len >> 1); p0 += 4 * L) {        // pair records p0, p0 + L, p0 + 2L, p0 + 3L: 8 candidates
            f32x2 d[4];
            bool any = false;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                d[u] = pair_sqdist(spts + (p0 + u * L) * 8, ux2, uy2, uz2);          // padded slots: +inf, never < b3
                any |= (d[u].x < b3) | (d[u].y < b3);
            }
            if (any) {                              // rare after warm-up
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    float dd = (u & 1) ? d[u >> 1].y : d[u >> 1].x;
                    if (dd < b3) {
                        int k = c0 + 2 * (p0 + (u >> 1) * L) + (u & 1);
                        if (dd < b1) { b3 = b2; i3 = i2; b2 = b1; i2 = i1; b1 = dd; i1 = k; }
                        else if (dd < b2) { b3 = b2; i3 = i2; b2 = dd; i2 = k; }
                        else { b3 = dd; i3 = k; }
                    }
                }
            }
        }
    }
    if (L > 1) {                                    // every lane of the wave takes part (a group never straddles waves)
        float r[3];
        int ri[3];
#pragma unroll
        for (int t = 0; t < 3; t++) {
            float d = b1;
            int k = i1;
#pragma unroll
            for (int s = 1; s < L; s <<= 1) {
                const float od = __shfl_xor(d, s, 64);
                const int ok = __shfl_xor(k, s, 64);
                const bool lt = od < d || (od == d && ok < k);
                d = lt ? od : d; k = lt ? ok : k;
            }
            r[t] = d; ri[t] = k;
            if (d < INFINITY && b1 == d && i1 == k) { b1 = b2; i1 = i2; b2 = b3; i2 = i3; b3 = INFINITY; i3 = 0; }
        }
        b1 = r[0]; b2 = r[1]; b3 = r[2];
        i1 = ri[0]; i2 = ri[1]; i3 = ri[2];
    }
    if (valid && l == 0) {
        // a query's three values are 12 contiguous bytes of each output: one 12-byte store per array (grid.hip)
        const size_t o = ((size_t)b * n + i) * 3;
        *reinterpret_cast<Trip<float>*>(dist2 + o) = Trip<float>{b1, b2, b3};
        *reinterpret_cast<Trip<int32_t>*>(idx + o) = Trip<int32_t>{i1, i2, i3};
        if (weight) {
            // PointnetFPModule: w = 1/(dist+1e-8), normalised
            // sqrtf and '/' are IEEE correctly rounded here (-fhip-fp32-correctly-rounded-divide-sqrt, set
            // explicitly in build.py); the __fsqrt_rn/__fdiv_rn intrinsics are NOT (they map to native ops).
            float r0 = 1.0f / (sqrtf(b1) + 1e-8f);
            float r1 = 1.0f / (sqrtf(b2) + 1e-8f);
            float r2 = 1.0f / (sqrtf(b3) + 1e-8f);
            float s = (r0 + r1) + r2;
            *reinterpret_cast<Trip<float>*>(weight + o) = Trip<float>{r0 / s, r1 / s, r2 / s};
        }
    }
}

// Lanes that share one query.  1 when the launch gives every SIMD of the chip (1 024) a wave of its own anyway; otherwise
// the smallest of 8 .. 64 that gives each SIMD two, as long as a lane still has 8 candidates to look at.
static int lanes_per_query(long queries, int candidates) {
    if (queries >= 65536) return 1;
    int L = 8;
    while (L < 64 && queries * L < 131072) L <<= 1;
    while (L > 8 && L * 8 > candidates) L >>= 1;
    return L;
}

template <int L>
static void launch_ball_query_lanes(const float* xyz, const float* new_xyz, int B, int N, int M, int seg_log2, float r2a, int nsa,
                                    int32_t* ia, float r2b, int nsb, int32_t* ib, bool dual, hipStream_t s) {
    dim3 grid(prcnn_divup(M, BQ_THREADS / L), B);
    if (dual)
        hipLaunchKernelGGL((ball_query_lanes_kernel<true, L>), grid, dim3(BQ_THREADS), 0, s, xyz, new_xyz, N, M, seg_log2, r2a, nsa, ia,
                           r2b, nsb, ib);
    else
        hipLaunchKernelGGL((ball_query_lanes_kernel<false, L>), grid, dim3(BQ_THREADS), 0, s, xyz, new_xyz, N, M, seg_log2, r2a, nsa, ia,
                           0.f, 0, (int32_t*)nullptr);
}

static int ball_query_impl(const float* xyz, const float* new_xyz, int B, int N, int M, float ra, int nsa, int32_t* ia,
                           float rb, int nsb, int32_t* ib, bool dual, hipStream_t s) {
    PRCNN_REQUIRE(B >= 0 && N > 0 && M >= 0 && nsa > 0 && (!dual || nsb > 0),
                  "prcnn_ball_query: bad shape B=%d N=%d M=%d nsample=%d/%d", B, N, M, nsa, nsb);
    if (B == 0 || M == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && new_xyz && ia && (!dual || ib), "prcnn_ball_query: null pointer");
    float r2a = ra * ra, r2b = rb * rb;        // fp32 product, as the oracle
    const int L = lanes_per_query((long)B * M, N);
    if (L > 1) {
        // candidates per lane and chunk: 8 .. 64 (one hit mask), the chunk no longer than the frame needs or the staging holds
        int seg_log2 = 3;
        while (seg_log2 < 6 && (L << seg_log2) < N && (L << seg_log2) < NB_CHUNK) seg_log2++;
        switch (L) {
            case 8: launch_ball_query_lanes<8>(xyz, new_xyz, B, N, M, seg_log2, r2a, nsa, ia, r2b, nsb, ib, dual, s); break;
            case 16: launch_ball_query_lanes<16>(xyz, new_xyz, B, N, M, seg_log2, r2a, nsa, ia, r2b, nsb, ib, dual, s); break;
            case 32: launch_ball_query_lanes<32>(xyz, new_xyz, B, N, M, seg_log2, r2a, nsa, ia, r2b, nsb, ib, dual, s); break;
            default: launch_ball_query_lanes<64>(xyz, new_xyz, B, N, M, seg_log2, r2a, nsa, ia, r2b, nsb, ib, dual, s); break;
        }
        PRCNN_LAUNCH_CHECK("prcnn_ball_query");
        return PRCNN_OK;
    }
    dim3 grid(prcnn_divup(M, BQ_THREADS), B);
    if (dual)
        hipLaunchKernelGGL(ball_query_kernel<true>, grid, dim3(BQ_THREADS), 0, s, xyz, new_xyz, N, M, r2a, nsa, ia, r2b,
                           nsb, ib);
    else
        hipLaunchKernelGGL(ball_query_kernel<false>, grid, dim3(BQ_THREADS), 0, s, xyz, new_xyz, N, M, r2a, nsa, ia,
                           0.f, 0, (int32_t*)nullptr);
    PRCNN_LAUNCH_CHECK("prcnn_ball_query");
    return PRCNN_OK;
}

PRCNN_API int prcnn_ball_query(const float* xyz, const float* new_xyz, int B, int N, int M, float radius, int nsample,
                               int32_t* idx, prcnn_stream_t stream) {
    return ball_query_impl(xyz, new_xyz, B, N, M, radius, nsample, idx, 0.f, 0, nullptr, false, (hipStream_t)stream);
}

PRCNN_API int prcnn_ball_query2(const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a,
                                int nsample_a, int32_t* idx_a, float radius_b, int nsample_b, int32_t* idx_b,
                                prcnn_stream_t stream) {
    return ball_query_impl(xyz, new_xyz, B, N, M, radius_a, nsample_a, idx_a, radius_b, nsample_b, idx_b, true,
                           (hipStream_t)stream);
}

template <int L>
static void launch_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                            float* weight, hipStream_t s) {
    hipLaunchKernelGGL(three_nn_kernel<L>, dim3(prcnn_divup(n, NN_THREADS / L), B), dim3(NN_THREADS), 0, s, unknown, known, n, m,
                       dist2, idx, weight);
}

PRCNN_API int prcnn_three_nn(const float* unknown, const float* known, int B, int n, int m, float* dist2, int32_t* idx,
                             float* weight, prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && n >= 0 && m > 0, "prcnn_three_nn: bad shape B=%d n=%d m=%d", B, n, m);
    if (B == 0 || n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(unknown && known && dist2 && idx, "prcnn_three_nn: null pointer");
    hipStream_t s = (hipStream_t)stream;
    switch (lanes_per_query((long)B * n, m)) {
        case 1: launch_three_nn<1>(unknown, known, B, n, m, dist2, idx, weight, s); break;
        case 8: launch_three_nn<8>(unknown, known, B, n, m, dist2, idx, weight, s); break;
        case 16: launch_three_nn<16>(unknown, known, B, n, m, dist2, idx, weight, s); break;
        case 32: launch_three_nn<32>(unknown, known, B, n, m, dist2, idx, weight, s); break;
        default: launch_three_nn<64>(unknown, known, B, n, m, dist2, idx, weight, s); break;
    }
    PRCNN_LAUNCH_CHECK("prcnn_three_nn");
    return PRCNN_OK;
}
