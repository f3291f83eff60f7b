// grid_layout.h -- per-frame neighbour grid as laid out in the caller's buffer (grid.hip builds and searches it), and the
// index-order ball-query scan of one 64-centroid block, shared by neighbor.hip's scan kernel and by grid.hip's grid kernel,
// whose workgroups run it themselves on the frames the header's density estimate flags as dense.
#pragma once
#include "common.h"

#define GRID_DIM_MAX 128                         // cells per axis: 64 (three_nn: ~1 known point per cell) or 128 (ball query:
#define GRID_CELLS_MAX (GRID_DIM_MAX * GRID_DIM_MAX)   //  crowded near-sensor cells stay small); buffers are sized for 128

struct GridHeader {
    float x0, z0, inv_cs, cs;
    int dim;                                      // cells per axis of THIS grid
    // Estimated candidates a ball query of radius min_cell visits: (points per occupied cell) x (cells its square of
    // cell columns overlaps).  A frame whose estimate exceeds N / 32 is DENSE: the per-thread sorted hit lists of the grid
    // kernel cost ~50x a scan's packed-fp32 pair test per candidate, so there the index-order scan (which also exits as soon
    // as both lists are full) is the faster exact method.  The grid kernel's workgroups of such a frame run that scan.
    float cand;
    int pad1, pad2;
};
// per-frame block inside the caller's buffer: header | cell_start[128*128 + 1] | sorted[N] float4
static inline size_t grid_frame_bytes(int N) {
    size_t b = sizeof(GridHeader) + (size_t)(GRID_CELLS_MAX + 1) * 4;
    b = (b + 15) & ~(size_t)15;
    return b + (size_t)N * 16;
}
__device__ __forceinline__ const GridHeader* grid_header(const void* g, size_t fb, int b) { return (const GridHeader*)((const char*)g + fb * b); }
__device__ __forceinline__ bool grid_frame_dense(const GridHeader& H, int N) { return H.cand > (float)N * (1.0f / 32.0f); }

// ---- the index-order scan (ball query and three_nn of neighbor.hip) ---------------------------------------------
#define BQ_THREADS 64       // ball query: ONE wave per workgroup -> wave-local staging, 4x more workgroups than 256-thread
                            // blocks (the op only has B*M threads in total), no cross-wave barrier in the scan
#define NB_CHUNK 1024       // candidates staged per LDS chunk: 512 pairs * 32 B = 16 KB
#define NB_CHUNK_BYTES (NB_CHUNK * 16)

// On CDNA4 only PACKED fp32 VALU ops (v_pk_add/mul_f32) run at the full 64 lanes x 2 rate; plain v_add/v_mul_f32
// measured ~3.6 cycles per wave64 instruction.  Candidates are therefore staged as PAIRS -- LDS record of pair p =
// {x0,x1,y0,y1 | z0,z1,-,-} (two ds_read_b128 broadcasts) -- and every distance evaluation below is a float2
// expression the compiler lowers to v_pk_*: same individually rounded operations per component, half the VALU issue.
typedef float f32x2 __attribute__((ext_vector_type(2)));

// LDS record of candidate pair p: floats [8p .. 8p+7] = {x0,x1,y0,y1,z0,z1,-,-}; point i of a chunk goes to pair i>>1, slot i&1.
// squared distances of the query to the two candidates of pair record `rec` (canonical arithmetic per component)
__device__ __forceinline__ f32x2 pair_sqdist(const float* rec, f32x2 qx, f32x2 qy, f32x2 qz) {
    float4 a = *reinterpret_cast<const float4*>(rec);          // x0 x1 y0 y1
    f32x2 z = *reinterpret_cast<const f32x2*>(rec + 4);        // z0 z1
    f32x2 dx = qx - (f32x2){a.x, a.y}, dy = qy - (f32x2){a.z, a.w}, dz = qz - z;
    return (dx * dx + dy * dy) + dz * dz;                       // -ffp-contract=off: no FMA, left to right
}

// candidates of a chunk that starts at c0 of `count`, rounded up to the step of the scans (8 candidates per lane that shares
// the query; a power of two that divides NB_CHUNK): the slots between the frame's end and that bound are staged as +inf, the
// slots past it are neither staged nor scanned
__device__ __forceinline__ int chunk_scan_len(int count, int c0, int step = 8) { return (min(NB_CHUNK, count - c0) + step - 1) & ~(step - 1); }

// three values of one query: 12 contiguous bytes of an output, written with one global_store_dwordx3
template <typename T> struct __attribute__((packed, aligned(4))) Trip { T a, b, c; };

// One wave (BQ_THREADS lanes, the whole workgroup) answers centroids [mblock * 64, +64) of frame b: lane = centroid, the
// frame streams through `spts` (NB_CHUNK_BYTES of LDS, 16-byte aligned) in ascending index order.
template <bool DUAL>
__device__ __forceinline__ void ball_query_scan_block(float* spts, const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                      int N, int M, int b, int mblock, float r2a, int nsa, int32_t* __restrict__ idxa,
                                                      float r2b, int nsb, int32_t* __restrict__ idxb) {
    const int tid = threadIdx.x;
    const int m = mblock * BQ_THREADS + tid;
    const bool valid = m < M;
    const float* __restrict__ p = xyz + (size_t)b * N * 3;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) {
        const float* q = new_xyz + ((size_t)b * M + m) * 3;
        qx = q[0]; qy = q[1]; qz = q[2];
    }
    const f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    int32_t* oa = idxa + ((size_t)b * M + (valid ? m : 0)) * nsa;
    int32_t* ob = DUAL ? idxb + ((size_t)b * M + (valid ? m : 0)) * nsb : nullptr;
    int cnta = 0, cntb = 0, firsta = 0, firstb = 0;
    const float r2max = DUAL ? fmaxf(r2a, r2b) : r2a;
    bool done = !valid;

    // The chunk for iteration c+1 is fetched into registers while chunk c is scanned: with one wave per workgroup
    // nothing else would hide the global-load latency of the staging.
    constexpr int PER_LANE = NB_CHUNK * 3 / BQ_THREADS;       // 48 floats of the flat xyz stream per lane per chunk
    float pre[PER_LANE];
    auto fetch_chunk = [&](int c0) {
        const int cnt3 = min(NB_CHUNK, N - c0) * 3, len3 = chunk_scan_len(N, c0) * 3;
        const float* src = p + (size_t)c0 * 3;
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int i = tid + u * BQ_THREADS;
            if (u * BQ_THREADS < len3) pre[u] = i < cnt3 ? src[i] : INFINITY;          // slots past the frame end: +inf, never a hit
        }
    };
    auto store_chunk = [&](int c0) {
        const int len3 = chunk_scan_len(N, c0) * 3;
#pragma unroll
        for (int u = 0; u < PER_LANE; u++) {
            int i = tid + u * BQ_THREADS;
            int pt = i / 3, c = i - pt * 3;
            if (i < len3) spts[(pt >> 1) * 8 + c * 2 + (pt & 1)] = pre[u];
        }
    };
    fetch_chunk(0);
    for (int c0 = 0; c0 < N; c0 += NB_CHUNK) {
        if (__all(done)) break;                    // single-wave workgroup: the whole block is finished
        __syncthreads();
        store_chunk(c0);
        __syncthreads();
        if (c0 + NB_CHUNK < N) fetch_chunk(c0 + NB_CHUNK);
        if (!done) {
            const int len = chunk_scan_len(N, c0);
            for (int i0 = 0; i0 < len; i0 += 8) {
                // 8 candidates = 4 packed pairs, ONE test for "any of them inside the larger ball"
                f32x2 d2[4];
                bool any = false;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    d2[u] = pair_sqdist(spts + (i0 / 2 + u) * 8, qx2, qy2, qz2);     // padded slots give +inf
                    any |= (d2[u].x < r2max) | (d2[u].y < r2max);
                }
                if (any) {
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        float d = (u & 1) ? d2[u >> 1].y : d2[u >> 1].x;
                        if (d < r2max) {
                            int k = c0 + i0 + u;
                            if (d < r2a && cnta < nsa) {
                                if (cnta == 0) firsta = k;
                                oa[cnta++] = k;
                            }
                            if (DUAL && d < r2b && cntb < nsb) {
                                if (cntb == 0) firstb = k;
                                ob[cntb++] = k;
                            }
                        }
                    }
                    if (cnta >= nsa && (!DUAL || cntb >= nsb)) { done = true; break; }
                }
            }
        }
    }
    if (valid) {
        for (int s = cnta; s < nsa; s++) oa[s] = firsta;      // pad with the first hit (0 if none)
        if (DUAL)
            for (int s = cntb; s < nsb; s++) ob[s] = firstb;
    }
}
