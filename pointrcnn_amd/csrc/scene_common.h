// scene_common.h -- what the two input builders share (scene.hip: inference branch, train_scene.hip: training branch): the
// lidar -> rect -> image projection with get_valid_flag, and the npoints draw (radix select, ties, LDS bitonic shuffle).
// The arithmetic contract and the random streams are stated in scene.hip's header comment.
#pragma once
#include "lds_sort.h"
#include "counter_rand.h"

constexpr int SCENE_THREADS = 1024;
constexpr int SCENE_MAX_TIES = 1024;
constexpr unsigned SCENE_FAR = 1u << 30;


struct RectPoint { float x, y, z; bool valid; };

// lidar -> rect (calibration.py:51-59) under the canonical contract; c = M, 4x3 row-major.  Shared with gt_database.hip.
__device__ __forceinline__ void scene_rect(const float4 p, const float* __restrict__ c, float& x, float& y, float& z) {
    x = ((p.x * c[0] + p.y * c[3]) + p.z * c[6]) + c[9];
    y = ((p.x * c[1] + p.y * c[4]) + p.z * c[7]) + c[10];
    z = ((p.x * c[2] + p.y * c[5]) + p.z * c[8]) + c[11];
}

__device__ __forceinline__ RectPoint scene_project(const float4 p, const float* __restrict__ c, int H, int W, const double* scope,
                                                   int use_scope) {
    RectPoint r;
    scene_rect(p, c, r.x, r.y, r.z);
    const float* P = c + 12;
    const float h0 = ((r.x * P[0] + r.y * P[1]) + r.z * P[2]) + P[3];
    const float h1 = ((r.x * P[4] + r.y * P[5]) + r.z * P[6]) + P[7];
    const float h2 = ((r.x * P[8] + r.y * P[9]) + r.z * P[10]) + P[11];
    const float u = h0 / r.z, v = h1 / r.z, depth = h2 - P[11];
    bool ok = (u >= 0.f) && (u < (float)W) && (v >= 0.f) && (v < (float)H) && (depth >= 0.f);
    if (use_scope)
        ok = ok && ((double)r.x >= scope[0]) && ((double)r.x <= scope[1]) && ((double)r.y >= scope[2]) && ((double)r.y <= scope[3]) &&
             ((double)r.z >= scope[4]) && ((double)r.z <= scope[5]);
    r.valid = ok;
    return r;
}

// block-wide: given this thread's histogram bin count c (1024 bins = 1024 threads), find the bin where the running count
// crosses `want` (0-based rank): returns the bin through sel[0] and the rank inside that bin through sel[1]
__device__ __forceinline__ void scene_pick_bin(int c, int want, int* wsum, int* sel) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; w++) before += wsum[w];
    const int hi = before + incl, lo = hi - c;
    if (c > 0 && lo <= want && want < hi) { sel[0] = tid; sel[1] = want - lo; }
    __syncthreads();
}


// block-wide (SCENE_THREADS threads): the draw and the shuffle of one frame.  L holds the frame's n candidates (f of them far) as
// (class | 30-bit key, identity); afterwards keys[lds_phys(0 .. total-1)] hold (shuffle key << 32 | identity) in output order.
// *nties and *nsel must have been zeroed by one thread (a barrier inside orders that write).  -> (total, status)
struct SceneSel { int total, status; };
__device__ __forceinline__ SceneSel scene_select_sort(const uint2* __restrict__ L, int n, int f, int np, int NP, unsigned seed, unsigned b,
                                                      u64* keys, int* hist, int* wsum, int* sel, unsigned* ties, int* nties, int* nsel) {
    const int tid = threadIdx.x;
    // what to draw: k candidates with the smallest keys; far points are outside the draw (always kept) when more valid
    // points than npoints exist, inside it otherwise (top-up from ALL valid points, kitti_rcnn_dataset.py:299-303)
    int st = 0, k;
    bool keep_far, keep_all;
    if (n > np) {
        keep_all = false;
        if (f > np) { st = 1; keep_far = false; k = np; }            // the reference's np.random.choice raises (negative size)
        else { keep_far = true; k = np - f; }
    } else {
        keep_all = true; keep_far = false;
        k = np - n;
        if (k > n) { st = 1; k = n; }                                // the reference raises (cannot draw k > n without replacement)
    }
    const int ncand = keep_far ? n - f : n;
    // ---- radix select: T = the k-th smallest 30-bit key among the candidates (rank k-1), need = how many of key == T to take
    unsigned T = 0;
    int need = 0;
    if (k > 0 && k < ncand) {
        unsigned prefix = 0;
        int want = k - 1;
        for (int pass = 0; pass < 3; pass++) {
            const int shift = 20 - 10 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int e = tid; e < n; e += SCENE_THREADS) {
                const unsigned code = L[e].x;
                if (keep_far && (code & SCENE_FAR)) continue;
                const unsigned key = code & (SCENE_FAR - 1u);
                if (pass == 0 || (key >> (shift + 10)) == prefix) atomicAdd(&hist[(key >> shift) & 1023u], 1);
            }
            __syncthreads();
            scene_pick_bin(hist[tid], want, wsum, sel);
            prefix = (prefix << 10) | (unsigned)sel[0];
            want = sel[1];
            __syncthreads();
        }
        T = prefix;
        need = want + 1;
    } else if (k >= ncand) {
        T = SCENE_FAR;                                   // every candidate key is < 2^30: take them all
    }                                                    // k == 0: T = 0, need = 0 -> none
    // ---- ties on key == T: the `need` smallest raw indices
    if (need > 0) {
        for (int e = tid; e < n; e += SCENE_THREADS) {
            const uint2 it = L[e];
            if (keep_far && (it.x & SCENE_FAR)) continue;
            if ((it.x & (SCENE_FAR - 1u)) == T) {
                const int p = atomicAdd(nties, 1);
                if (p < SCENE_MAX_TIES) ties[p] = it.y;
            }
        }
    }
    __syncthreads();
    const int m = min(*nties, SCENE_MAX_TIES);
    // ---- gather the selection into LDS as (shuffle key << 32 | raw index)
    for (int e0 = 0; e0 < n; e0 += SCENE_THREADS) {
        const int e = e0 + tid;
        if (e < n) {
            const uint2 it = L[e];
            const bool isfar = (it.x & SCENE_FAR) != 0u;
            const unsigned key = it.x & (SCENE_FAR - 1u);
            const bool cand = !(keep_far && isfar);
            bool drawn = cand && key < T;
            if (cand && need > 0 && key == T) {
                int rank = 0;
                for (int q = 0; q < m; q++) rank += ties[q] < it.y ? 1 : 0;
                drawn = rank < need;
            }
            if (keep_all || (keep_far && isfar)) {
                const int p = atomicAdd(nsel, 1);
                keys[lds_phys(p)] = ((u64)scene_rand(seed, 1u, b, it.y) << 32) | it.y;
            }
            if (drawn) {
                const int p = atomicAdd(nsel, 1);
                keys[lds_phys(p)] = ((u64)scene_rand(seed, keep_all ? 2u : 1u, b, it.y) << 32) | it.y;
            }
        }
    }
    __syncthreads();
    const int total = *nsel;                               // == npoints unless st == 1
    u64 v[16];
    if (tid * 16 < NP) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int j = tid * 16 + e;
            v[e] = j < total ? keys[lds_phys(j)] : ~0ULL;
        }
    }
    __syncthreads();
    block_sort16(v, keys, NP, tid);
    SceneSel r;
    r.total = total; r.status = st;
    return r;
}
