// scene_common.h -- the one home of what the passes over raw velodyne frames share.  Users: scene.hip (inference input),
// train_scene.hip (RPN training batch), gt_database.hip (GT-augmentation database: the rect transform and the frame checks).
// A new pass takes its prelude from here:
//   device  SceneFrames (head of the kernel params), scene_rect / scene_project (lidar -> rect -> image, get_valid_flag),
//           scene_append (a block's valid points -> the frame's candidate list), SceneLds + scene_draw + scene_gather (the npoints
//           draw: radix select, ties, the selection as shuffle keys), scene_select_sort (draw + LDS bitonic shuffle, npoints <= 16384),
//           scene_select_large (draw -> the frame's HBM key array, npoints > 16384), scene_large_identity (row j's identity after
//           the HBM sort), scene_empty_frame (the rows of a frame without candidates);
//   host    scene_check_frames, scene_fill_frames (scope, NP, the counters | list workspace), scene_fill_large (the key arrays and
//           per-frame totals behind it), scene_reset_counters, scene_launch_sample, scene_large_shuffle (the HBM sort, scene.hip)
//           -- each takes the entry point's name (`who`) for its messages.
// The arithmetic contract and the random streams are stated in scene.hip's header comment.
#pragma once
#include "lds_sort.h"
#include "counter_rand.h"

constexpr int SCENE_THREADS = 1024;
constexpr int SCENE_MAX_TIES = 1024;
constexpr unsigned SCENE_FAR = 1u << 30;
constexpr int SCENE_SMALL_MAX = 16384;       // npoints up to here: draw and shuffle in one workgroup's LDS
constexpr int SCENE_LARGE_MAX = 65536;       // npoints up to here: the shuffle sorts SCENE_SMALL_MAX-key chunks through HBM

// head of the kernel params of a pass that draws npoints of every frame: SceneParams and TrainSceneParams derive from it
struct SceneFrames {
    const float4* raw;          // (total, 4) x y z intensity, lidar frame
    const int64_t* off;         // (B+1) first raw point of every frame
    const float* calib;         // (B, 24): M (4x3 row-major), P2 (3x4 row-major)
    const int32_t* img_hw;      // (B, 2) image height, width
    double scope[6];            // x0 x1 y0 y1 z0 z1 (PC_AREA_SCOPE)
    int use_scope;
    int B, npoints, NP;         // NP: npoints rounded up to a power of two >= 16, what the shuffle sorts
    unsigned seed;
    uint2* list;                // candidate entries (class | 30-bit key, identity); where frame b starts is the pass's own layout
    int32_t* counters;          // (B, 2) candidates, far ones -- zeroed by scene_reset_counters
    float* out_xyz;             // (B, npoints, 3)
    int32_t* out_src;           // (B, npoints) identity of every output point
    int32_t* nvalid;            // (B)
    int32_t* status;            // (B) 0 ok, 1 outside the reference's domain (it raises), 2 no valid point
    u64* large_keys;            // npoints > SCENE_SMALL_MAX only: (B, NP) shuffle keys, sorted through HBM between select and rows
    int32_t* large_total;       // (B) keys a frame selected (0: the frame wrote its empty rows in the select launch)
};

struct RectPoint { float x, y, z; bool valid; };

// lidar -> rect (calibration.py:51-59) under the canonical contract; c = M, 4x3 row-major
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

// block-wide (SCENE_THREADS threads, one point i of frame b each): the valid points are appended, unordered, to the frame's
// candidate list as (far bit | 30-bit draw key, i), with one atomic per block on each of the frame's two counters
__device__ __forceinline__ void scene_append(bool valid, bool far, int i, uint2* list, int32_t* counters_b, unsigned seed, int b) {
    __shared__ int wv[SCENE_THREADS / 64], wf[SCENE_THREADS / 64];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long bv = __ballot(valid), bf = __ballot(far);
    if (lane == 0) { wv[wave] = (int)__popcll(bv); wf[wave] = (int)__popcll(bf); }
    __syncthreads();
    if (tid == 0) {
        int tv = 0, tf = 0;
        for (int w = 0; w < SCENE_THREADS / 64; w++) { tv += wv[w]; tf += wf[w]; }
        base = tv > 0 ? atomicAdd(counters_b, tv) : 0;
        if (tf > 0) atomicAdd(counters_b + 1, tf);
    }
    __syncthreads();
    if (valid) {
        int pos = base + (int)__popcll(bv & ((1ULL << lane) - 1ULL));
        for (int w = 0; w < wave; w++) pos += wv[w];
        const unsigned key = scene_rand(seed, 0u, (unsigned)b, (unsigned)i) >> 2;
        list[pos] = make_uint2(key | (far ? SCENE_FAR : 0u), (unsigned)i);
    }
}

// the static LDS of the draw; a sample kernel declares one, __shared__, next to the dynamic `keys`
struct SceneLds {
    int hist[1024];
    int wsum[SCENE_THREADS / 64];
    int sel[2];
    unsigned ties[SCENE_MAX_TIES];
    int nties, nsel;
};

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

// block-wide (SCENE_THREADS threads): the draw of one frame.  L holds the frame's n > 0 candidates (f of them far) as
// (class | 30-bit key, identity).  -> what scene_gather needs to tell the selected candidates; the tie list is left in S.
struct SceneDraw {
    int status, need, m;        // need of the m listed candidates with key == T belong to the draw
    unsigned T;
    bool keep_far, keep_all;
};
__device__ __forceinline__ SceneDraw scene_draw(const uint2* __restrict__ L, int n, int f, int np, SceneLds& S) {
    const int tid = threadIdx.x;
    if (tid == 0) { S.nties = 0; S.nsel = 0; }           // ordered before their first use by the barriers below
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
            S.hist[tid] = 0;
            __syncthreads();
            for (int e = tid; e < n; e += SCENE_THREADS) {
                const unsigned code = L[e].x;
                if (keep_far && (code & SCENE_FAR)) continue;
                const unsigned key = code & (SCENE_FAR - 1u);
                if (pass == 0 || (key >> (shift + 10)) == prefix) atomicAdd(&S.hist[(key >> shift) & 1023u], 1);
            }
            __syncthreads();
            scene_pick_bin(S.hist[tid], want, S.wsum, S.sel);
            prefix = (prefix << 10) | (unsigned)S.sel[0];
            want = S.sel[1];
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
                const int p = atomicAdd(&S.nties, 1);
                if (p < SCENE_MAX_TIES) S.ties[p] = it.y;
            }
        }
    }
    __syncthreads();
    SceneDraw D;
    D.status = st; D.need = need; D.m = min(S.nties, SCENE_MAX_TIES); D.T = T; D.keep_far = keep_far; D.keep_all = keep_all;
    return D;
}

// block-wide, after scene_draw: hands every selected candidate to put(slot, shuffle key << 32 | identity), the slots 0 .. total-1
// in the order the atomics append (the sort that follows removes it).  -> total (== npoints unless D.status == 1)
template <class Put>
__device__ __forceinline__ int scene_gather(const uint2* __restrict__ L, int n, const SceneDraw& D, unsigned seed, unsigned b, SceneLds& S, Put put) {
    const int tid = threadIdx.x;
    for (int e0 = 0; e0 < n; e0 += SCENE_THREADS) {
        const int e = e0 + tid;
        if (e < n) {
            const uint2 it = L[e];
            const bool isfar = (it.x & SCENE_FAR) != 0u;
            const unsigned key = it.x & (SCENE_FAR - 1u);
            const bool cand = !(D.keep_far && isfar);
            bool drawn = cand && key < D.T;
            if (cand && D.need > 0 && key == D.T) {
                int rank = 0;
                for (int q = 0; q < D.m; q++) rank += S.ties[q] < it.y ? 1 : 0;
                drawn = rank < D.need;
            }
            if (D.keep_all || (D.keep_far && isfar)) put(atomicAdd(&S.nsel, 1), ((u64)scene_rand(seed, 1u, b, it.y) << 32) | it.y);
            if (drawn) put(atomicAdd(&S.nsel, 1), ((u64)scene_rand(seed, D.keep_all ? 2u : 1u, b, it.y) << 32) | it.y);
        }
    }
    __syncthreads();
    return S.nsel;
}

// block-wide (SCENE_THREADS threads): the draw and the shuffle of one frame with npoints <= SCENE_SMALL_MAX; afterwards
// keys[lds_phys(0 .. total-1)] hold (shuffle key << 32 | identity) in output order.  -> (total, status)
struct SceneSel { int total, status; };
__device__ __forceinline__ SceneSel scene_select_sort(const uint2* __restrict__ L, int n, int f, int np, int NP, unsigned seed, unsigned b,
                                                      u64* keys, SceneLds& S) {
    const int tid = threadIdx.x;
    const SceneDraw D = scene_draw(L, n, f, np, S);
    const int total = scene_gather(L, n, D, seed, b, S, [keys](int p, u64 v) { keys[lds_phys(p)] = v; });
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
    r.total = total; r.status = D.status;
    return r;
}

// block-wide: frame b has no candidate: zero rows, source -1, status 2.  feat = the pass's (B, npoints) feature output,
// in4 = its optional (B, npoints, 4) input output (NULL: none)
__device__ __forceinline__ void scene_empty_frame(const SceneFrames& F, int b, float* feat, float* in4) {
    const size_t row0 = (size_t)b * F.npoints;
    for (size_t j = row0 + threadIdx.x; j < row0 + F.npoints; j += SCENE_THREADS) {
        F.out_xyz[j * 3] = 0.f; F.out_xyz[j * 3 + 1] = 0.f; F.out_xyz[j * 3 + 2] = 0.f; feat[j] = 0.f; F.out_src[j] = -1;
        if (in4) { in4[j * 4] = 0.f; in4[j * 4 + 1] = 0.f; in4[j * 4 + 2] = 0.f; in4[j * 4 + 3] = 0.f; }
    }
    if (threadIdx.x == 0) F.status[b] = 2;
}

// block-wide, npoints > SCENE_SMALL_MAX: the draw of frame b (L: its candidate list) into the frame's NP-entry key array, unsorted,
// the tail [total, NP) filled with ~0; nvalid, status and the frame's total are written here.  A frame without candidates writes
// its empty rows and total 0: the sort and row launches skip it.  feat / in4 as scene_empty_frame.
__device__ __forceinline__ void scene_select_large(const SceneFrames& F, int b, const uint2* __restrict__ L, float* feat, float* in4, SceneLds& S) {
    const int tid = threadIdx.x;
    const int n = F.counters[b * 2], f = F.counters[b * 2 + 1];
    if (tid == 0) F.nvalid[b] = n;
    if (n == 0) {
        scene_empty_frame(F, b, feat, in4);
        if (tid == 0) F.large_total[b] = 0;
        return;
    }
    u64* keys = F.large_keys + (size_t)b * F.NP;
    const SceneDraw D = scene_draw(L, n, f, F.npoints, S);
    const int total = scene_gather(L, n, D, F.seed, (unsigned)b, S, [keys](int p, u64 v) { keys[p] = v; });
    for (int j = total + tid; j < F.NP; j += SCENE_THREADS) keys[j] = ~0ULL;
    if (tid == 0) { F.large_total[b] = total; F.status[b] = D.status; }
}

// identity of output row j < npoints of frame b once the key array is sorted (a short selection -- status 1 -- repeats cyclically);
// only entries below total are read, so the padding identity 0xFFFFFFFF never becomes an address.  total > 0.
__device__ __forceinline__ unsigned scene_large_identity(const SceneFrames& F, int b, int j, int total) {
    return (unsigned)F.large_keys[(size_t)b * F.NP + (j < total ? j : j % total)];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
// What every pass requires of the frames it is given.  `threads` = the block size of its per-point kernel, extra_per_frame = what
// the pass adds to a frame's candidates.  With B == 0, or idle (nothing to do whatever the frames hold), the pointers may be NULL.
// A guard on the frames themselves (offsets that do not describe raw, a bound on B) belongs here.
static int scene_check_frames(const char* who, const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                              const float* calib, long extra_per_frame, int threads, bool idle = false) {
    PRCNN_REQUIRE(B >= 0 && total_points >= 0 && max_points_per_frame >= 0, "%s: bad shape B=%d total=%ld", who, B, (long)total_points);
    if (B == 0 || idle) return PRCNN_OK;
    PRCNN_REQUIRE(offsets && calib, "%s: null pointer", who);
    PRCNN_REQUIRE(total_points == 0 || raw, "%s: null raw points", who);
    PRCNN_REQUIRE(((uintptr_t)raw % 16) == 0, "%s: raw points must be 16-byte aligned", who);
    PRCNN_REQUIRE((long)max_points_per_frame + extra_per_frame < (1L << 31) - threads, "%s: frame too large", who);
    return PRCNN_OK;
}

// the workspace of a drawing pass is  counters (B, 2) | candidate list, the list on the next 64-byte boundary
static size_t scene_counters_bytes(int B) { return (size_t)B * 2 * sizeof(int32_t); }
static size_t scene_list_offset(int B) { return ((scene_counters_bytes(B) + 63) / 64) * 64; }
static int scene_pow2(int npoints) { int NP = 16; while (NP < npoints) NP <<= 1; return NP; }      // what the shuffle sorts

static void scene_fill_frames(SceneFrames& F, const float* raw, const int64_t* offsets, int B, const float* calib, const int32_t* img_hw,
                              const double* scope, int npoints, uint32_t seed, void* workspace, float* out_xyz, int32_t* out_src,
                              int32_t* nvalid, int32_t* status) {
    F.raw = reinterpret_cast<const float4*>(raw); F.off = offsets; F.calib = calib; F.img_hw = img_hw;
    F.use_scope = scope != nullptr;
    for (int q = 0; q < 6; q++) F.scope[q] = scope ? scope[q] : 0.0;
    F.B = B; F.npoints = npoints; F.seed = seed;
    F.NP = scene_pow2(npoints);
    F.counters = static_cast<int32_t*>(workspace);
    F.list = reinterpret_cast<uint2*>(static_cast<char*>(workspace) + scene_list_offset(B));
    F.out_xyz = out_xyz; F.out_src = out_src; F.nvalid = nvalid; F.status = status;
}

// Behind a pass's small-form workspace (small_bytes of it), for npoints > SCENE_SMALL_MAX:  key arrays (B, NP) u64 on the next
// 256-byte boundary | totals (B) i32
static size_t scene_large_offset(size_t small_bytes) { return ((small_bytes + 255) / 256) * 256; }
static size_t scene_large_bytes(size_t small_bytes, int B, int npoints) {
    if (npoints <= SCENE_SMALL_MAX) return small_bytes;
    return scene_large_offset(small_bytes) + (size_t)B * scene_pow2(npoints) * sizeof(u64) + (size_t)B * sizeof(int32_t);
}
static void scene_fill_large(SceneFrames& F, void* workspace, size_t small_bytes) {
    char* base = static_cast<char*>(workspace) + scene_large_offset(small_bytes);
    F.large_keys = reinterpret_cast<u64*>(base);
    F.large_total = reinterpret_cast<int32_t*>(base + (size_t)F.B * F.NP * sizeof(u64));
}
// the exact ascending sort of every frame's NP keys through HBM, in plain launches on s (scene.hip)
int scene_large_shuffle(const char* who, const SceneFrames& F, hipStream_t s);

static int scene_reset_counters(const char* who, const SceneFrames& F, hipStream_t s) {
    if (prcnn_fill_words(F.counters, 0u, (size_t)F.B * 2, s) != hipSuccess) return prcnn_fail(PRCNN_EHIP, "%s: memset failed", who);
    return PRCNN_OK;
}

// one SCENE_THREADS workgroup per frame with the LDS of the NP-key sort; the first launch on a device raises the kernel's limit
template <auto KERNEL, class Params>
static int scene_launch_sample(const char* who, const Params& P, hipStream_t s) {
    static PrcnnLdsLimit attr;
    if (!attr.raise((const void*)KERNEL, (int)lds_sort_bytes(16384))) return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", who);
    hipLaunchKernelGGL(KERNEL, dim3(P.B), dim3(SCENE_THREADS), lds_sort_bytes(P.NP), s, P);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return prcnn_fail(PRCNN_EHIP, "%s(sample): launch failed: %s", who, hipGetErrorString(e));
    return PRCNN_OK;
}
