// proposal.hip -- the proposal stage between the RPN heads and roipool3d, batched and sync-free on gfx950.
//
// Replaces:
//   lib/utils/bbox_transform.py:24-121   decode_bbox_target      -> decode_kernel
//   lib/rpn/proposal_layer.py:35-141     ProposalLayer.forward   -> sort_split_kernel + greedy_nms_kernel + assemble_kernel
//   tools/eval_rcnn.py:600-614           per-frame score select + rotated NMS -> sort_split_kernel + greedy_nms_kernel
//
// The reference runs this stage as a Python loop over frames: per frame ~20 tiny torch kernels, two blocking
// iou3d_cuda.nms_* calls (each: N x N/64 mask kernel, synchronous D2H copy of the mask, host sweep; iou3d.cpp:86-116)
// and boolean-mask indexing that synchronises the host on every dist_mask.sum().  Here the whole batch is three
// launches and nothing ever returns to the host:
//   sort_split_kernel : one workgroup per frame; 64-bit (score, index) keys bitonic-sorted in LDS (16 K keys = 136 KB of
//                       the CU's 160 KB), then a block scan splits the ordered list into the distance areas.
//   greedy_nms_kernel : one workgroup per (frame, area).  A box only ever needs testing against KEPT earlier boxes, and
//                       at most post_top_n (70 / 30) are kept, so the N^2/2 pair matrix of the reference (19.8 M IoUs
//                       per 6300-box call) is never formed: <= N x post_top_n pair tests, no mask in HBM.
//   assemble_kernel   : concatenates the two areas' survivors into the zero-padded (B, post, 7) / (B, post) outputs.
// Arithmetic follows oracle/prcnn_oracle.c (prcnn_cpu_decode_bbox_target / prcnn_cpu_proposal_layer /
// prcnn_cpu_nms_batched) operation for operation; results are bit-identical to it.
#include "iou3d_geom.h"
#include "lds_sort.h"
#include "switches.h"

// ====================================================================================================
// decode_bbox_target
// ====================================================================================================
struct DecodeParams {
    const float* roi;
    const float* reg;
    float* out;
    long N;
    int roi_cols, C;
    int nb, nyb, nhb;
    int x_res_l, z_res_l, y_bin_l, y_res_l, y_off, ry_bin_l, ry_res_l, size_l;
    int get_xz_fine, get_y_by_bin, get_ry_fine, y_to_bottom;
    float lbs, half_lbs, scope, lybs, half_lybs, yscope;
    float apc, half_apc, quarter_pi, pi, two_pi;
    float anchor[3];
};

__device__ __forceinline__ int argmax_first(const float* v, int n) {      // torch.argmax: first maximum, NaN maximal
    int best = 0;
    for (int i = 1; i < n; i++) {
        if (v[best] != v[best]) break;
        if (v[i] > v[best] || v[i] != v[i]) best = i;
    }
    return best;
}

// One workgroup per 64 rows: its four waves read the (64, C) slab with unit-stride loads into LDS (row stride C|1 words, so
// the per-lane row walks below are bank-conflict free) -- all of a thread's loads are issued before the first LDS store, and
// LDS (not the wave count) bounds residency, so four loading waves per slab put four times the bytes in flight of one -- then
// the first wave decodes a row per lane.
#define DEC_THREADS 256
__global__ __launch_bounds__(DEC_THREADS) void decode_kernel(DecodeParams P) {
    extern __shared__ float rows[];
    const int tid = threadIdx.x, lane = tid;
    const long row0 = (long)blockIdx.x * 64;
    const int nrows = (int)min(64L, P.N - row0);
    const int C = P.C, ld = C | 1;
    const float* __restrict__ src = P.reg + row0 * C;
    const int total = nrows * C;
    if ((C & 3) == 0 && ((uintptr_t)P.reg & 15) == 0) {      // 16-byte loads; a float4 never straddles two rows
        constexpr int U = 5;                                  // 64 x 76 floats = 4.75 float4 per thread
        for (int e0 = tid * 4; e0 < total; e0 += U * DEC_THREADS * 4) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = e0 + u * DEC_THREADS * 4;
                if (e < total) v[u] = *reinterpret_cast<const float4*>(src + e);
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int e = e0 + u * DEC_THREADS * 4;
                if (e < total) {
                    const int r = e / C, c = e - r * C;
                    float* d = rows + r * ld + c;
                    d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
                }
            }
        }
    } else {
        int r = 0, c = tid;
        while (c >= C) { c -= C; r++; }
        for (int e = tid; e < total; e += DEC_THREADS) {
            rows[r * ld + c] = src[e];
            c += DEC_THREADS;
            while (c >= C) { c -= C; r++; }
        }
    }
    __syncthreads();
    if (lane >= nrows) return;
    const float* rg = rows + lane * ld;
    const float* b = P.roi + (row0 + lane) * P.roi_cols;
    const int xb = argmax_first(rg, P.nb), zb = argmax_first(rg + P.nb, P.nb);
    float px = sub(add(mul((float)xb, P.lbs), P.half_lbs), P.scope);                   // bbox_transform.py:53-54
    float pz = sub(add(mul((float)zb, P.lbs), P.half_lbs), P.scope);
    if (P.get_xz_fine) {                                                               // :56-67
        px = add(px, mul(rg[P.x_res_l + xb], P.lbs));
        pz = add(pz, mul(rg[P.z_res_l + zb], P.lbs));
    }
    float py;
    if (P.get_y_by_bin) {                                                              // :70-79
        int yb = argmax_first(rg + P.y_bin_l, P.nyb);
        float y_res = mul(rg[P.y_res_l + yb], P.lybs);
        py = add(sub(add(mul((float)yb, P.lybs), P.half_lybs), P.yscope), y_res);
        py = add(py, b[1]);
    } else {
        py = add(b[1], rg[P.y_off]);                                                   // :84
    }
    const int rb = argmax_first(rg + P.ry_bin_l, P.nhb);
    const float ry_res = mul(rg[P.ry_res_l + rb], P.half_apc);
    float ry;
    if (P.get_ry_fine) {                                                               // :92-96
        ry = sub(add(add(mul((float)rb, P.apc), P.half_apc), ry_res), P.quarter_pi);
    } else {                                                                           // :97-103
        float a = add(mul((float)rb, P.apc), ry_res);
        float m = fmodf(a, P.two_pi);                                                  // torch.remainder
        if (m != 0.0f && m < 0.0f) m = add(m, P.two_pi);
        ry = m > P.pi ? sub(m, P.two_pi) : m;
    }
    const float h = add(mul(rg[P.size_l], P.anchor[0]), P.anchor[0]);                  // :109-110
    const float w = add(mul(rg[P.size_l + 1], P.anchor[1]), P.anchor[1]);
    const float l = add(mul(rg[P.size_l + 2], P.anchor[2]), P.anchor[2]);
    if (P.roi_cols == 7) {                                                             // :116-119, rotate by -roi_ry
        const float ang = -b[6];
        const float ca = (float)cos((double)ang), sa = (float)sin((double)ang);
        const float nx = add(mul(px, ca), mul(pz, -sa));
        const float nz = add(mul(px, sa), mul(pz, ca));
        px = nx; pz = nz;
        ry = add(ry, b[6]);
    }
    px = add(px, b[0]);                                                                // :120
    pz = add(pz, b[2]);
    if (P.y_to_bottom) py = add(py, h / 2);                                            // proposal_layer.py:32
    float* o = P.out + (row0 + lane) * 7;
    o[0] = px; o[1] = py; o[2] = pz; o[3] = h; o[4] = w; o[5] = l; o[6] = ry;
}

// ====================================================================================================
// score sort + area split
// ====================================================================================================
#define SPLIT_ALL 0      // score_based_proposal: every row is a candidate
#define SPLIT_RANGE 1    // distance_based_proposal: area 1 = (r0, r1], area 2 = (r1, r2] on box z
#define SPLIT_VALID 2    // final detection select: rows with valid[b, i] != 0

struct SortParams {
    const float* scores;     // (B, N)
    const float* boxes3d;    // (B, N, 7)  (SPLIT_RANGE)
    const uint8_t* valid;    // (B, N)     (SPLIT_VALID)
    int32_t* cand;           // (B, nseg, cand_ld) candidate row indices, descending score
    int32_t* cnt;            // (B, nseg)
    int N, Npad, mode, nseg, cand_ld;
    int pre1, pre2;
    float r0, r1, r2;
};

// descending score, NaN first, -0 == +0, ties by ascending index  ==  ascending 64-bit key
__device__ __forceinline__ u64 sort_key(float s, int idx) {
    s = s + 0.0f;
    unsigned u = __float_as_uint(s);
    unsigned ok = (s != s) ? 0xFFFFFFFFu : ((u & 0x80000000u) ? ~u : (u | 0x80000000u));
    return ((u64)(~ok) << 32) | (unsigned)idx;
}

__global__ __launch_bounds__(1024) void sort_split_kernel(SortParams P) {
    extern __shared__ u64 keys[];                       // lds_phys(Npad) keys, then 40 words of scan scratch
    const int b = blockIdx.x, t = threadIdx.x, T = blockDim.x;
    const int N = P.N, Npad = P.Npad;
    const int nact = Npad >> 4;                         // threads that own 16 keys
    const bool active = t < nact;
    unsigned* scratch = (unsigned*)(keys + lds_phys(Npad) + 1);
    u64 v[16];
    if (active) {
        const float* __restrict__ sc = P.scores + (size_t)b * N;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const int i = t * 16 + e;
            v[e] = i < N ? sort_key(sc[i], i) : ~0ULL;
        }
    }
    block_sort16(v, keys, Npad, t);
    // ---- split the ordered list into areas (proposal_layer.py:78-98): per-thread flags, block exclusive scan ----
    unsigned f1 = 0, f2 = 0;
    int idx[16];
    if (active) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const u64 key = v[e];
            idx[e] = (int)(unsigned)key;
            if (key == ~0ULL) { idx[e] = -1; continue; }
            if (P.mode == SPLIT_RANGE) {
                const float z = P.boxes3d[((size_t)b * N + idx[e]) * 7 + 2];
                if (z > P.r0 && z <= P.r1) f1 |= 1u << e;
                if (z > P.r1 && z <= P.r2) f2 |= 1u << e;
            } else if (P.mode == SPLIT_VALID) {
                if (P.valid[(size_t)b * N + idx[e]]) f1 |= 1u << e;
            } else {
                f1 |= 1u << e;
            }
        }
    }
    const unsigned mine = (unsigned)__popc(f1) | ((unsigned)__popc(f2) << 16);    // both counts <= 16384 < 2^16
    unsigned inc = mine;
    const int lane = t & 63, wave = t >> 6, nwaves = T >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) scratch[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        unsigned w = lane < nwaves ? scratch[lane] : 0u, winc = w;
#pragma unroll
        for (int d = 1; d < 16; d <<= 1) {
            unsigned o = __shfl_up(winc, d, 64);
            if (lane >= d) winc += o;
        }
        if (lane < nwaves) scratch[16 + lane] = winc - w;          // exclusive wave offsets
        if (lane == nwaves - 1) scratch[32] = winc;                // totals
    }
    __syncthreads();
    const unsigned excl = scratch[16 + wave] + inc - mine;
    const unsigned tot = scratch[32];
    const int n1 = (int)(tot & 0xFFFFu), n2 = (int)(tot >> 16);
    int32_t* c1 = P.cand + (size_t)b * P.nseg * P.cand_ld;
    int32_t* c2 = c1 + P.cand_ld;
    const bool borrow = P.mode == SPLIT_RANGE && n2 == 0;           // area 2 empty: ranks [pre1, pre1+pre2) of area 1
    if (active) {
        int r1 = (int)(excl & 0xFFFFu), r2 = (int)(excl >> 16);
#pragma unroll
        for (int e = 0; e < 16; e++) {
            if ((f1 >> e) & 1u) {
                if (r1 < P.pre1) c1[r1] = idx[e];
                else if (borrow && r1 - P.pre1 < P.pre2) c2[r1 - P.pre1] = idx[e];
                r1++;
            }
            if ((f2 >> e) & 1u) {
                if (r2 < P.pre2) c2[r2] = idx[e];
                r2++;
            }
        }
    }
    if (t == 0) {
        P.cnt[b * P.nseg] = min(n1, P.pre1);
        if (P.nseg > 1) P.cnt[b * P.nseg + 1] = borrow ? max(0, min(n1 - P.pre1, P.pre2)) : min(n2, P.pre2);
    }
}

// ---- frames with more than 16384 rows: the same bitonic network, spilled to HBM between LDS-sized chunks -----------
// 16384-key chunks are sorted in LDS (chunk c ascending when (c & 1) == 0, else descending: the bitonic building blocks),
// every later stage k does its strides >= 16384 as a global compare-exchange pass and its strides < 16384 as one LDS merge
// per chunk.  A descending sort / merge is an ascending one on the complemented keys.
#define LARGE_CHUNK 16384
__global__ __launch_bounds__(1024) void large_local_sort_kernel(const float* __restrict__ scores, int N, int Ntot, u64* __restrict__ ws) {
    extern __shared__ u64 keys[];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const float* __restrict__ sc = scores + (size_t)b * N;
    const bool desc = c & 1;
    u64 v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const int i = c * LARGE_CHUNK + t * 16 + e;
        const u64 k = i < N ? sort_key(sc[i], i) : ~0ULL;
        v[e] = desc ? ~k : k;
    }
    block_sort16(v, keys, LARGE_CHUNK, t);
    u64* o = ws + (size_t)b * Ntot + (size_t)c * LARGE_CHUNK + t * 16;
#pragma unroll
    for (int e = 0; e < 16; e++) o[e] = desc ? ~v[e] : v[e];
}
__global__ __launch_bounds__(256) void large_cx_kernel(u64* __restrict__ ws, int Ntot, int j, int k) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (Ntot >> 1)) return;
    u64* w = ws + (size_t)b * Ntot;
    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    const u64 a = w[i], c = w[i + j];
    const bool up = (i & k) == 0;
    if ((a > c) == up) { w[i] = c; w[i + j] = a; }
}
__global__ __launch_bounds__(1024) void large_local_merge_kernel(u64* __restrict__ ws, int Ntot, int k) {
    extern __shared__ u64 keys[];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const bool desc = ((c * LARGE_CHUNK) & k) != 0;
    u64* o = ws + (size_t)b * Ntot + (size_t)c * LARGE_CHUNK + t * 16;
    u64 v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = desc ? ~o[e] : o[e];
    block_merge16(v, keys, LARGE_CHUNK, t);
#pragma unroll
    for (int e = 0; e < 16; e++) o[e] = desc ? ~v[e] : v[e];
}
// area split over the HBM-resident order: pass 0 counts, pass 1 writes (the borrow rule needs the far area's total first)
__global__ __launch_bounds__(1024) void large_split_kernel(SortParams P, const u64* __restrict__ ws, int Ntot) {
    __shared__ unsigned scratch[40];
    const int b = blockIdx.x, t = threadIdx.x, N = P.N;
    const int lane = t & 63, wave = t >> 6;
    const u64* __restrict__ w = ws + (size_t)b * Ntot;
    int32_t* c1 = P.cand + (size_t)b * P.nseg * P.cand_ld;
    int32_t* c2 = c1 + P.cand_ld;
    int tot1 = 0, tot2 = 0;
    bool borrow = false;
    for (int pass = 0; pass < 2; pass++) {
        int run1 = 0, run2 = 0;
        for (int base = 0; base < Ntot; base += LARGE_CHUNK) {
            unsigned f1 = 0, f2 = 0;
            int idx[16];
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const u64 key = w[base + t * 16 + e];
                idx[e] = (int)(unsigned)key;
                if (key == ~0ULL) continue;
                if (P.mode == SPLIT_RANGE) {
                    const float z = P.boxes3d[((size_t)b * N + idx[e]) * 7 + 2];
                    if (z > P.r0 && z <= P.r1) f1 |= 1u << e;
                    if (z > P.r1 && z <= P.r2) f2 |= 1u << e;
                } else if (P.mode == SPLIT_VALID) {
                    if (P.valid[(size_t)b * N + idx[e]]) f1 |= 1u << e;
                } else {
                    f1 |= 1u << e;
                }
            }
            const unsigned mine = (unsigned)__popc(f1) | ((unsigned)__popc(f2) << 16);
            unsigned inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                unsigned o = __shfl_up(inc, d, 64);
                if (lane >= d) inc += o;
            }
            __syncthreads();
            if (lane == 63) scratch[wave] = inc;
            __syncthreads();
            if (wave == 0) {
                unsigned wv = lane < 16 ? scratch[lane] : 0u, winc = wv;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    unsigned o = __shfl_up(winc, d, 64);
                    if (lane >= d) winc += o;
                }
                if (lane < 16) scratch[16 + lane] = winc - wv;
                if (lane == 15) scratch[32] = winc;
            }
            __syncthreads();
            const unsigned excl = scratch[16 + wave] + inc - mine, tot = scratch[32];
            if (pass == 1) {
                int r1 = run1 + (int)(excl & 0xFFFFu), r2 = run2 + (int)(excl >> 16);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    if ((f1 >> e) & 1u) {
                        if (r1 < P.pre1) c1[r1] = idx[e];
                        else if (borrow && r1 - P.pre1 < P.pre2) c2[r1 - P.pre1] = idx[e];
                        r1++;
                    }
                    if ((f2 >> e) & 1u) {
                        if (r2 < P.pre2) c2[r2] = idx[e];
                        r2++;
                    }
                }
            }
            run1 += (int)(tot & 0xFFFFu);
            run2 += (int)(tot >> 16);
        }
        if (pass == 0) { tot1 = run1; tot2 = run2; borrow = P.mode == SPLIT_RANGE && tot2 == 0; }
    }
    if (t == 0) {
        P.cnt[b * P.nseg] = min(tot1, P.pre1);
        if (P.nseg > 1) P.cnt[b * P.nseg + 1] = borrow ? max(0, min(tot1 - P.pre1, P.pre2)) : min(tot2, P.pre2);
    }
}

// ====================================================================================================
// greedy NMS against the kept list
// ====================================================================================================
struct NBox { float v[5]; };
template <int KIND> struct BoxOf { typedef RBox type; };
template <> struct BoxOf<PRCNN_NMS_NORMAL> { typedef NBox type; };

__device__ __forceinline__ void to_bev(const float* __restrict__ b, float (&v)[5]) {      // kitti_utils.py:134-147
    const float half_l = b[5] / 2, half_w = b[4] / 2;
    v[0] = sub(b[0], half_l); v[1] = sub(b[2], half_w); v[2] = add(b[0], half_l); v[3] = add(b[2], half_w); v[4] = b[6];
}
__device__ __forceinline__ void make_box(const float (&v)[5], RBox& r) { make_rbox(v, r); }
__device__ __forceinline__ void make_box(const float (&v)[5], NBox& r) {
#pragma unroll
    for (int c = 0; c < 5; c++) r.v[c] = v[c];
}
// does the earlier (higher-score) box suppress the later one?  iou3d_kernel.cu:284-286 / :339-341
__device__ __forceinline__ bool suppresses(const RBox& earlier, const RBox& later, float thresh) {
    if (thresh >= 0.0f && decided_without_clip(earlier, later, thresh)) return false;       // overlap exactly 0, or provably below the threshold
    return iou_bev(earlier, later) > thresh;
}
__device__ __forceinline__ bool suppresses(const NBox& earlier, const NBox& later, float thresh) {
    return iou_normal(earlier.v, later.v) > thresh;
}

struct NmsParams {
    const float* boxes3d;    // (B, N, 7)
    const int32_t* cand;     // (B, nseg, cand_ld)
    const int32_t* cnt;      // (B, nseg)
    int32_t* kept;           // (B, nseg, kept_ld): kept row indices in kept order, -1 padded up to max_keep
    int32_t* kept_cnt;       // (B, nseg)
    int N, nseg, cand_ld, kept_ld;
    int post1, post2;
    float thresh;
};

#define NMS_THREADS 256
#define PAIR_CAP 4096        // pair-list entries (rotated): one 64 x 32 tile of (kept, candidate) pairs is 2048
template <int KIND>
static size_t greedy_nms_lds_bytes(int max_keep) {
    return 64 * sizeof(u64) + 4 * sizeof(u64) + 4 * sizeof(int) + (KIND == PRCNN_NMS_ROTATED ? PAIR_CAP * sizeof(unsigned) : 0) +
           (size_t)(64 + max_keep) * sizeof(typename BoxOf<KIND>::type);
}

// wave-aggregated append of `code` for the lanes with pass == true
__device__ __forceinline__ void push_pairs(bool pass, unsigned code, unsigned* list, int* count) {
    const u64 bm = __ballot(pass);
    if (bm == 0ULL) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(count, (int)__popcll(bm));
    base = __builtin_amdgcn_readfirstlane(base);
    if (pass) list[base + __popcll(bm & ((1ULL << lane) - 1ULL))] = code;
}
__device__ __forceinline__ void set_bit(u64* word, int bit) { atomicOr((unsigned*)word + (bit >> 5), 1u << (bit & 31)); }

// Candidates are taken 64 at a time.  A: every candidate is tested against the kept list; B: the surviving
// candidates' 64x64 upper triangle; C: wave 0 resolves the chunk serially on uniform 64-bit masks (as the reference's
// host sweep does per word, iou3d.cpp:103-116) and appends the survivors.
//   NORMAL : the IoU is a dozen flops, so A and B evaluate every pair directly (A: the 4 waves split the kept list;
//            B: one row per ballot).
//   ROTATED: a polygon clip costs thousands of instructions and almost every pair is far apart, so A and B first run
//            the circumscribed-circle test over all pairs (far_apart: exact-zero overlap), compact the few that pass
//            into an LDS list, and spread THOSE over all 256 threads -- the expensive evaluations run at full lane
//            occupancy instead of one divergent lane per row.
template <int KIND>
__global__ __launch_bounds__(NMS_THREADS) void greedy_nms_kernel(NmsParams P) {
    typedef typename BoxOf<KIND>::type Box;
    constexpr bool ROT = KIND == PRCNN_NMS_ROTATED;
    extern __shared__ u64 smem64[];
    u64* m = smem64;                                    // [64] chunk suppression rows
    u64* supw = m + 64;                                 // [4]  phase-A hits (NORMAL: one word per wave; ROTATED: word 0)
    int* sh = (int*)(supw + 4);                         // [0] running kept count, [1] pair-list length
    unsigned* pairs = (unsigned*)(sh + 4);
    Box* cand = (Box*)(pairs + (ROT ? PAIR_CAP : 0));
    Box* keptb = cand + 64;
    const int seg = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = seg ? P.post2 : P.post1;
    const size_t sb = (size_t)b * P.nseg + seg;
    const int32_t* __restrict__ cl = P.cand + sb * P.cand_ld;
    int32_t* kept_out = P.kept + sb * P.kept_ld;
    const int n = P.cnt[sb];
    const float* __restrict__ boxes = P.boxes3d + (size_t)b * P.N * 7;
    const float thresh = P.thresh;
    const bool prefilter = thresh >= 0.0f;              // a zero overlap can only suppress when thresh < 0
    int nk = 0;
    for (int c0 = 0; c0 < n && nk < K; c0 += 64) {
        const int nc = min(64, n - c0);
        if (tid < nc) {
            float v[5];
            to_bev(boxes + (size_t)cl[c0 + tid] * 7, v);
            make_box(v, cand[tid]);
        }
        if (tid < 64) m[tid] = 0ULL;
        if (tid < 4) supw[tid] = 0ULL;
        if (tid == 0) sh[1] = 0;
        __syncthreads();
        // ---- A: candidates vs kept list ----
        if constexpr (ROT) {
            for (int k0 = 0; k0 < nk; k0 += 32) {
                const int nt = min(32, nk - k0);
#pragma unroll 2
                for (int q = tid; q < 64 * 32; q += NMS_THREADS) {
                    const int c = q & 63, kk = q >> 6;
                    bool pass = kk < nt && c < nc;
                    if (pass && prefilter) pass = !decided_without_clip(keptb[k0 + kk], cand[c], thresh);
                    push_pairs(pass, ((unsigned)(k0 + kk) << 6) | (unsigned)c, pairs, &sh[1]);
                }
                __syncthreads();
                const int np = sh[1];
                __syncthreads();                                          // everyone has read np before the next tile appends
                if (k0 + 32 >= nk || np > PAIR_CAP - 64 * 32) {           // flush: evaluate what has been collected
                    for (int e = tid; e < np; e += NMS_THREADS) {
                        const unsigned code = pairs[e];
                        const int c = code & 63, k = code >> 6;
                        if ((supw[0] >> c) & 1ULL) continue;              // already suppressed by another kept box
                        if (iou_bev(keptb[k], cand[c]) > thresh) set_bit(&supw[0], c);
                    }
                    __syncthreads();
                    if (tid == 0) sh[1] = 0;
                    __syncthreads();
                }
            }
        } else {
            bool hit = false;
            if (lane < nc)
                for (int k = wave; k < nk && !hit; k += 4) hit = suppresses(keptb[k], cand[lane], thresh);
            const u64 hm = __ballot(hit);
            if (lane == 0) supw[wave] = hm;
            __syncthreads();
        }
        const u64 validm = nc == 64 ? ~0ULL : ((1ULL << nc) - 1ULL);
        const u64 alive = validm & ~(supw[0] | supw[1] | supw[2] | supw[3]);
        // ---- B: upper triangle among the surviving candidates ----
        if constexpr (ROT) {
#pragma unroll 2
            for (int q = tid; q < 64 * 64; q += NMS_THREADS) {
                const int c = q & 63, r = q >> 6;
                bool pass = r < c && ((alive >> r) & 1ULL) && ((alive >> c) & 1ULL);
                if (pass && prefilter) pass = !decided_without_clip(cand[r], cand[c], thresh);
                push_pairs(pass, ((unsigned)r << 6) | (unsigned)c, pairs, &sh[1]);   // <= 2016 entries
            }
            __syncthreads();
            const int np = sh[1];
            for (int e = tid; e < np; e += NMS_THREADS) {
                const unsigned code = pairs[e];
                const int c = code & 63, r = code >> 6;
                if (iou_bev(cand[r], cand[c]) > thresh) set_bit(&m[r], c);
            }
        } else {
            for (int rr = 0; rr < 16; rr++) {
                const int r = wave * 16 + rr;
                bool h = false;
                if (((alive >> r) & 1ULL) && lane > r && ((alive >> lane) & 1ULL)) h = suppresses(cand[r], cand[lane], thresh);
                const u64 bm = __ballot(h);
                if (lane == 0) m[r] = bm;
            }
        }
        __syncthreads();
        if (wave == 0) {                                // ---- C ----
            const u64 row = m[lane];
            const unsigned rlo = (unsigned)row, rhi = (unsigned)(row >> 32);
            u64 cur = ~alive, keptm = 0ULL;
            int num = nk;
            for (int t = 0; t < nc; t++) {
                if (num == K) break;
                if (!((cur >> t) & 1ULL)) {
                    keptm |= 1ULL << t;
                    num++;
                    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)rlo, t);
                    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)rhi, t);
                    cur |= ((u64)hi << 32) | lo;
                }
            }
            if ((keptm >> lane) & 1ULL) {
                const int pos = nk + __popcll(keptm & ((1ULL << lane) - 1ULL));
                keptb[pos] = cand[lane];
                kept_out[pos] = cl[c0 + lane];
            }
            if (lane == 0) sh[0] = num;
        }
        __syncthreads();
        nk = sh[0];
    }
    if (tid == 0) P.kept_cnt[sb] = nk;
    for (int k = nk + tid; k < K; k += NMS_THREADS) kept_out[k] = -1;
}

// ----------------------------------------------------------------------------------------------------
// Rotated greedy NMS with a PREFILTER (round 5).  On a driving scene almost every candidate is a vote for a car whose
// best box is already kept: in greedy_nms_kernel every chunk of 64 such candidates costs the full serial step (load, A, B, C)
// although none of them survives phase A -- ~40 steps of ~65 us before 70 boxes of a 24-car scene are kept.  Here a batch of
// NMS_PB raw candidates (one per thread) is tested against the kept list first, every thread walking the kept list on its own
// candidate: the nearest kept box that can overlap first, then the others in order -- the cheap circle test skips to the next
// kept box that can overlap, then ALL threads that found one clip together (a round costs one polygon clip whatever the number
// of lanes in it; a candidate leaves at its first suppressing box).  Only the survivors -- in score order -- go through the chunk step (A' against the boxes kept since the batch's
// prefilter, B among themselves, C the serial resolve), so the serial steps are per 64 SURVIVORS, not per 64 candidates.
// The decisions are the same IoU tests on the same operands as greedy_nms_kernel<ROTATED> makes (a candidate is dropped iff
// some earlier kept box has IoU > thresh with it; kept boxes are never un-kept): identical keep lists (PRCNN_NMS_PREFILTER=0
// selects the chunk kernel; tests/test_gpu_proposal.py compares both with the oracle).
// ----------------------------------------------------------------------------------------------------
#define NMS_RT 1024          // threads of the prefiltered kernel: four waves per SIMD (the polygon clip waits on its private arrays; 256: 2.15 ms, 512: 1.35 ms, 1024: 1.23 ms)
#define NMS_PB NMS_RT
#ifndef NMS_PB0
#define NMS_PB0 64          // the first batch
#endif
#ifndef NMS_PBG
#define NMS_PBG 4           // growth from batch to batch (first batch 64 / 128 / 256 / 1024: 832 / 851 / 853 / 1098 us for the bs32 rotated proposal layer; growth 2 / 4 / 8 / 16: 932 / 832 / 836 / 831)
#endif
static size_t greedy_nms_rot_lds_bytes(int max_keep) {
    return 64 * sizeof(u64) + 4 * sizeof(u64) + 32 * sizeof(int) + PAIR_CAP * sizeof(unsigned) + NMS_PB * sizeof(int) +
           (size_t)(64 + NMS_PB + max_keep) * sizeof(RBox);
}

__global__ __launch_bounds__(NMS_RT) void greedy_nms_rot_kernel(NmsParams P) {
    extern __shared__ u64 smem64[];
    u64* m = smem64;                                    // [64] chunk suppression rows
    u64* supw = m + 64;                                 // [0] phase-A' hits
    int* sh = (int*)(supw + 4);                         // [0] running kept count, [1] pair-list length, [8..23] survivors per wave
    unsigned* pairs = (unsigned*)(sh + 32);
    int* surv = (int*)(pairs + PAIR_CAP);               // [NMS_PB] batch positions of the survivors, in score order
    RBox* cand = (RBox*)(surv + NMS_PB);                // [64] the chunk
    RBox* pre = cand + 64;                              // [NMS_PB] the batch
    RBox* keptb = pre + NMS_PB;
    const int seg = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = seg ? P.post2 : P.post1;
    const size_t sb = (size_t)b * P.nseg + seg;
    const int32_t* __restrict__ cl = P.cand + sb * P.cand_ld;
    int32_t* kept_out = P.kept + sb * P.kept_ld;
    const int n = P.cnt[sb];
    const float* __restrict__ boxes = P.boxes3d + (size_t)b * P.N * 7;
    const float thresh = P.thresh;
    const bool prefilter = thresh >= 0.0f;              // a zero overlap can only suppress when thresh < 0
    int nk = 0;
    // Round 6: the batches GROW (64, 256, 1024, 1024, ...).  The first batch meets an empty kept list, so all of it goes through the
    // serial chunk steps: with 1024 candidates up front that was 16 steps (~2/3 of the kernel) spent on votes for the ~24 cars the
    // first few chunks keep.  A short first batch keeps the best box of most cars in ONE step; the next, four times as long, is
    // prefiltered against those.  The batch size is free: survivors go through the chunk steps in score order whatever it is.
    int pb = NMS_PB0;
    for (int p0 = 0; p0 < n && nk < K; p0 += pb, pb = min(NMS_PB, pb * NMS_PBG)) {
        const int nb = min(pb, n - p0);
        const int nk0 = nk;                             // the kept list this batch is prefiltered against
        // ---- prefilter: my candidate against kept[0, nk0) ----
        bool alive = tid < nb;
        if (alive) {
            float v[5];
            to_bev(boxes + (size_t)cl[p0 + tid] * 7, v);
            make_rbox(v, pre[tid]);
        }
        __syncthreads();                                // (also: the previous batch's last chunk is done with cand / m / sh)
        {
            const RBox& me = pre[tid < nb ? tid : 0];
            // the nearest kept box that can overlap goes first: a vote for a car is almost always suppressed by the kept box closest to it,
            // so most candidates leave after ONE clip (the outcome is an OR over the kept boxes: the order of the tests is free)
            int kbest = -1;
            if (alive) {
                float dbest = 3.0e38f;
                for (int k = 0; k < nk0; k++) {
                    if (prefilter && decided_without_clip(keptb[k], me, thresh)) continue;
                    const float dx = sub(keptb[k].cx, me.cx), dy = sub(keptb[k].cy, me.cy);
                    const float d = add(mul(dx, dx), mul(dy, dy));
                    if (kbest < 0 || d < dbest) { dbest = d; kbest = k; }
                }
            }
            if (kbest >= 0 && iou_bev(keptb[kbest], me) > thresh) alive = false;
            int k = 0;
            bool scanning = alive && kbest >= 0;
            while (__any(scanning)) {
                if (scanning) {
                    while (k < nk0 && (k == kbest || (prefilter && decided_without_clip(keptb[k], me, thresh)))) k++;
                    scanning = k < nk0;
                }
                if (scanning) {
                    if (iou_bev(keptb[k], me) > thresh) { alive = false; scanning = false; }
                    k++;
                }
            }
        }
        // ---- survivors, in score order ----
        const u64 am = __ballot(alive);
        if (lane == 0) sh[8 + wave] = (int)__popcll(am);
        __syncthreads();
        int base = 0;
        for (int w = 0; w < wave; w++) base += sh[8 + w];
        int ns = 0;
        for (int w = 0; w < NMS_RT / 64; w++) ns += sh[8 + w];
        if (alive) surv[base + (int)__popcll(am & ((1ULL << lane) - 1ULL))] = tid;
        __syncthreads();
        // ---- chunks of 64 survivors ----
        for (int s0 = 0; s0 < ns && nk < K; s0 += 64) {
            const int nc = min(64, ns - s0);
            if (tid < nc) cand[tid] = pre[surv[s0 + tid]];
            if (tid < 64) m[tid] = 0ULL;
            if (tid == 0) { supw[0] = 0ULL; sh[1] = 0; }
            __syncthreads();
            // A': the chunk against the boxes kept since the prefilter (earlier chunks of this batch)
            for (int k0 = nk0; k0 < nk; k0 += 32) {
                const int nt = min(32, nk - k0);
#pragma unroll 2
                for (int q = tid; q < 64 * 32; q += NMS_RT) {
                    const int c = q & 63, kk = q >> 6;
                    bool pass = kk < nt && c < nc;
                    if (pass && prefilter) pass = !decided_without_clip(keptb[k0 + kk], cand[c], thresh);
                    push_pairs(pass, ((unsigned)(k0 + kk) << 6) | (unsigned)c, pairs, &sh[1]);
                }
                __syncthreads();
                const int np = sh[1];
                __syncthreads();
                if (k0 + 32 >= nk || np > PAIR_CAP - 64 * 32) {
                    for (int e = tid; e < np; e += NMS_RT) {
                        const unsigned code = pairs[e];
                        const int c = code & 63, k = code >> 6;
                        if ((supw[0] >> c) & 1ULL) continue;
                        if (iou_bev(keptb[k], cand[c]) > thresh) set_bit(&supw[0], c);
                    }
                    __syncthreads();
                    if (tid == 0) sh[1] = 0;
                    __syncthreads();
                }
            }
            const u64 validm = nc == 64 ? ~0ULL : ((1ULL << nc) - 1ULL);
            const u64 live = validm & ~supw[0];
            // B: upper triangle among the chunk
#pragma unroll 2
            for (int q = tid; q < 64 * 64; q += NMS_RT) {
                const int c = q & 63, r = q >> 6;
                bool pass = r < c && ((live >> r) & 1ULL) && ((live >> c) & 1ULL);
                if (pass && prefilter) pass = !decided_without_clip(cand[r], cand[c], thresh);
                push_pairs(pass, ((unsigned)r << 6) | (unsigned)c, pairs, &sh[1]);   // <= 2016 entries
            }
            __syncthreads();
            const int np = sh[1];
            for (int e = tid; e < np; e += NMS_RT) {
                const unsigned code = pairs[e];
                const int c = code & 63, r = code >> 6;
                if (iou_bev(cand[r], cand[c]) > thresh) set_bit(&m[r], c);
            }
            __syncthreads();
            if (wave == 0) {                            // C: serial resolve on uniform masks
                const u64 row = m[lane];
                const unsigned rlo = (unsigned)row, rhi = (unsigned)(row >> 32);
                u64 cur = ~live, keptm = 0ULL;
                int num = nk;
                for (int t = 0; t < nc; t++) {
                    if (num == K) break;
                    if (!((cur >> t) & 1ULL)) {
                        keptm |= 1ULL << t;
                        num++;
                        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)rlo, t);
                        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)rhi, t);
                        cur |= ((u64)hi << 32) | lo;
                    }
                }
                if ((keptm >> lane) & 1ULL) {
                    const int pos = nk + __popcll(keptm & ((1ULL << lane) - 1ULL));
                    keptb[pos] = cand[lane];
                    kept_out[pos] = cl[p0 + surv[s0 + lane]];
                }
                if (lane == 0) sh[0] = num;
            }
            __syncthreads();
            nk = sh[0];
        }
    }
    if (tid == 0) P.kept_cnt[sb] = nk;
    for (int k = nk + tid; k < K; k += NMS_RT) kept_out[k] = -1;
}

// ----------------------------------------------------------------------------------------------------
// The same prefilter for axis-aligned NMS (round 6).  greedy_nms_kernel<NORMAL> takes the candidates 64 at a time through the serial
// chunk step -- ~100 steps for 6 300 candidates although a handful of them keeps anything: 379 us of a 490 us proposal layer, on the
// DEFAULT path (RPN.NMS_TYPE 'normal').  Here a growing batch (64, 256, 1024, ...) is tested against the kept list first, one
// candidate per thread (an IoU is a dozen flops: a candidate walks the whole list in ~2 k instructions), and only the survivors, in score
// order, go through the chunk step (A' against the boxes kept since the batch's prefilter, B among themselves, C the serial resolve).
// Same tests on the same operands (iou_normal > thresh against every earlier kept box): identical keep lists; PRCNN_NMS_PREFILTER=0
// selects the chunk kernel.
// ----------------------------------------------------------------------------------------------------
static size_t greedy_nms_pre_lds_bytes(int max_keep) {
    return 64 * sizeof(u64) + 4 * sizeof(u64) + 32 * sizeof(int) + NMS_PB * sizeof(int) + (size_t)(64 + NMS_PB + max_keep) * sizeof(NBox);
}

__global__ __launch_bounds__(NMS_RT) void greedy_nms_pre_kernel(NmsParams P) {
    extern __shared__ u64 smem64[];
    u64* m = smem64;                                    // [64] chunk suppression rows
    u64* supw = m + 64;                                 // [0] phase-A' hits
    int* sh = (int*)(supw + 4);                         // [0] running kept count, [8..] survivors per wave
    int* surv = sh + 16 + 16;                           // [NMS_PB] batch positions of the survivors, in score order
    NBox* cand = (NBox*)(surv + NMS_PB);                // [64] the chunk
    NBox* pre = cand + 64;                              // [NMS_PB] the batch
    NBox* keptb = pre + NMS_PB;
    const int seg = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = seg ? P.post2 : P.post1;
    const size_t sb = (size_t)b * P.nseg + seg;
    const int32_t* __restrict__ cl = P.cand + sb * P.cand_ld;
    int32_t* kept_out = P.kept + sb * P.kept_ld;
    const int n = P.cnt[sb];
    const float* __restrict__ boxes = P.boxes3d + (size_t)b * P.N * 7;
    const float thresh = P.thresh;
    int nk = 0;
    int pb = NMS_PB0;
    for (int p0 = 0; p0 < n && nk < K; p0 += pb, pb = min(NMS_PB, pb * NMS_PBG)) {
        const int nb = min(pb, n - p0);
        const int nk0 = nk;                             // the kept list this batch is prefiltered against
        bool alive = tid < nb;
        NBox me;
        if (alive) {
            to_bev(boxes + (size_t)cl[p0 + tid] * 7, me.v);
            pre[tid] = me;
            for (int k = 0; k < nk0; k++)
                if (iou_normal(keptb[k].v, me.v) > thresh) { alive = false; break; }
        }
        // ---- survivors, in score order ----
        const u64 am = __ballot(alive);
        if (lane == 0) sh[8 + wave] = (int)__popcll(am);
        __syncthreads();                                // (also: pre[] is complete, the previous batch's last chunk is done with cand / m / sh)
        int base = 0;
        for (int w = 0; w < wave; w++) base += sh[8 + w];
        int ns = 0;
        for (int w = 0; w < NMS_RT / 64; w++) ns += sh[8 + w];
        if (alive) surv[base + (int)__popcll(am & ((1ULL << lane) - 1ULL))] = tid;
        __syncthreads();
        // ---- chunks of 64 survivors ----
        for (int s0 = 0; s0 < ns && nk < K; s0 += 64) {
            const int nc = min(64, ns - s0);
            if (tid < nc) cand[tid] = pre[surv[s0 + tid]];
            if (tid < 64) m[tid] = 0ULL;
            if (tid == 0) supw[0] = 0ULL;
            __syncthreads();
            // A': the chunk against the boxes kept since the prefilter (earlier chunks of this batch)
            for (int q = tid; q < 64 * (nk - nk0); q += NMS_RT) {
                const int c = q & 63, k = nk0 + (q >> 6);
                if (c < nc && iou_normal(keptb[k].v, cand[c].v) > thresh) set_bit(&supw[0], c);
            }
            __syncthreads();
            const u64 validm = nc == 64 ? ~0ULL : ((1ULL << nc) - 1ULL);
            const u64 live = validm & ~supw[0];
            // B: upper triangle among the chunk
            for (int q = tid; q < 64 * 64; q += NMS_RT) {
                const int c = q & 63, r = q >> 6;
                if (r < c && ((live >> r) & 1ULL) && ((live >> c) & 1ULL) && iou_normal(cand[r].v, cand[c].v) > thresh) set_bit(&m[r], c);
            }
            __syncthreads();
            if (wave == 0) {                            // C: serial resolve on uniform masks
                const u64 row = m[lane];
                const unsigned rlo = (unsigned)row, rhi = (unsigned)(row >> 32);
                u64 cur = ~live, keptm = 0ULL;
                int num = nk;
                for (int t = 0; t < nc; t++) {
                    if (num == K) break;
                    if (!((cur >> t) & 1ULL)) {
                        keptm |= 1ULL << t;
                        num++;
                        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)rlo, t);
                        const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)rhi, t);
                        cur |= ((u64)hi << 32) | lo;
                    }
                }
                if ((keptm >> lane) & 1ULL) {
                    const int pos = nk + __popcll(keptm & ((1ULL << lane) - 1ULL));
                    keptb[pos] = cand[lane];
                    kept_out[pos] = cl[p0 + surv[s0 + lane]];
                }
                if (lane == 0) sh[0] = num;
            }
            __syncthreads();
            nk = sh[0];
        }
    }
    if (tid == 0) P.kept_cnt[sb] = nk;
    for (int k = nk + tid; k < K; k += NMS_RT) kept_out[k] = -1;
}

// ====================================================================================================
// output assembly (proposal_layer.py:38-56,114-117)
// ====================================================================================================
struct AssembleParams {
    const float* scores;
    const float* boxes3d;
    const int32_t* kept;
    const int32_t* kept_cnt;
    float* out_boxes;
    float* out_scores;
    int32_t* out_count;
    int N, kept_ld, post;
};
__global__ __launch_bounds__(128) void assemble_kernel(AssembleParams P) {
    const int b = blockIdx.x;
    const int n1 = P.kept_cnt[b * 2], n2 = P.kept_cnt[b * 2 + 1];
    const int32_t* k1 = P.kept + (size_t)b * 2 * P.kept_ld;
    const int32_t* k2 = k1 + P.kept_ld;
    for (int slot = threadIdx.x; slot < P.post; slot += blockDim.x) {
        const int src = slot < n1 ? k1[slot] : (slot < n1 + n2 ? k2[slot - n1] : -1);
        float* ob = P.out_boxes + ((size_t)b * P.post + slot) * 7;
        if (src >= 0) {
            const float* ib = P.boxes3d + ((size_t)b * P.N + src) * 7;
#pragma unroll
            for (int c = 0; c < 7; c++) ob[c] = ib[c];
            P.out_scores[(size_t)b * P.post + slot] = P.scores[(size_t)b * P.N + src];
        } else {
#pragma unroll
            for (int c = 0; c < 7; c++) ob[c] = 0.0f;
            P.out_scores[(size_t)b * P.post + slot] = 0.0f;
        }
    }
    if (threadIdx.x == 0 && P.out_count) P.out_count[b] = n1 + n2;
}

// ====================================================================================================
// host side
// ====================================================================================================
#define PROPOSAL_MAX_SORT 16384
#define LDS_BUDGET (150 * 1024)

static int pow2_at_least(int n, int lo) {
    int p = lo;
    while (p < n) p <<= 1;
    return p;
}

PRCNN_API int prcnn_decode_bbox_target(const float* roi, int roi_cols, const float* pred_reg, long N, int C, double loc_scope,
                                       double loc_bin_size, int num_head_bin, const float* anchor_size_host, int get_xz_fine,
                                       int get_y_by_bin, double loc_y_scope, double loc_y_bin_size, int get_ry_fine,
                                       int y_to_bottom, float* out, prcnn_stream_t stream) {
    PRCNN_REQUIRE(N >= 0 && C > 0, "prcnn_decode_bbox_target: bad N=%ld C=%d", N, C);
    PRCNN_REQUIRE(roi_cols == 3 || roi_cols == 7, "prcnn_decode_bbox_target: roi_cols must be 3 (xyz) or 7 (boxes), got %d", roi_cols);
    PRCNN_REQUIRE(loc_bin_size > 0 && loc_y_bin_size > 0 && num_head_bin > 0 && anchor_size_host,
                  "prcnn_decode_bbox_target: bad bin configuration");
    DecodeParams P;
    P.nb = (int)(loc_scope / loc_bin_size) * 2;            // bbox_transform.py:42-43
    P.nyb = (int)(loc_y_scope / loc_y_bin_size) * 2;
    int off = P.nb * 2;
    P.x_res_l = P.nb * 2; P.z_res_l = P.nb * 3;
    if (get_xz_fine) off = P.nb * 4;
    P.y_bin_l = P.y_res_l = P.y_off = 0;
    if (get_y_by_bin) { P.y_bin_l = off; P.y_res_l = off + P.nyb; off += 2 * P.nyb; } else { P.y_off = off; off += 1; }
    P.ry_bin_l = off; P.ry_res_l = off + num_head_bin; P.size_l = off + 2 * num_head_bin;
    PRCNN_REQUIRE(P.nb > 0 && P.size_l + 3 == C, "prcnn_decode_bbox_target: C=%d does not match the bin layout (%d channels expected)",
                  C, P.size_l + 3);                        // the reference asserts (:106)
    if (N == 0) return PRCNN_OK;
    PRCNN_REQUIRE(roi && pred_reg && out, "prcnn_decode_bbox_target: null pointer");
    const double PI = 3.141592653589793;
    const double apc = get_ry_fine ? (PI / 2) / num_head_bin : (2 * PI) / num_head_bin;
    P.roi = roi; P.reg = pred_reg; P.out = out; P.N = N; P.roi_cols = roi_cols; P.C = C; P.nhb = num_head_bin;
    P.get_xz_fine = get_xz_fine; P.get_y_by_bin = get_y_by_bin; P.get_ry_fine = get_ry_fine; P.y_to_bottom = y_to_bottom;
    P.lbs = (float)loc_bin_size; P.half_lbs = (float)(loc_bin_size / 2); P.scope = (float)loc_scope;
    P.lybs = (float)loc_y_bin_size; P.half_lybs = (float)(loc_y_bin_size / 2); P.yscope = (float)loc_y_scope;
    P.apc = (float)apc; P.half_apc = (float)(apc / 2); P.quarter_pi = (float)(PI / 4); P.pi = (float)PI; P.two_pi = (float)(2 * PI);
    for (int c = 0; c < 3; c++) P.anchor[c] = anchor_size_host[c];
    const size_t lds = (size_t)64 * (C | 1) * sizeof(float);
    PRCNN_REQUIRE(lds <= 64 * 1024, "prcnn_decode_bbox_target: C=%d too wide", C);
    hipLaunchKernelGGL(decode_kernel, dim3(prcnn_divup(N, 64)), dim3(DEC_THREADS), lds, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_decode_bbox_target");
    return PRCNN_OK;
}

static size_t large_sort_bytes(int B, int N) {
    if (N <= PROPOSAL_MAX_SORT) return 0;
    return (size_t)B * (size_t)pow2_at_least(N, LARGE_CHUNK) * sizeof(u64);
}

static int launch_sort_split(const char* op, SortParams& P, int B, hipStream_t s, u64* large_ws) {
    if (P.N > PROPOSAL_MAX_SORT) {
        const int Ntot = pow2_at_least(P.N, LARGE_CHUNK), nchunks = Ntot / LARGE_CHUNK;
        static PrcnnLdsLimit attr_sort, attr_merge;
        if (!attr_sort.raise((const void*)large_local_sort_kernel, LDS_BUDGET) || !attr_merge.raise((const void*)large_local_merge_kernel, LDS_BUDGET))
            return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", op);
        const size_t lds = lds_sort_bytes(LARGE_CHUNK);
        hipLaunchKernelGGL(large_local_sort_kernel, dim3(nchunks, B), dim3(1024), lds, s, P.scores, P.N, Ntot, large_ws);
        for (int k = 2 * LARGE_CHUNK; k <= Ntot; k <<= 1) {
            for (int j = k >> 1; j >= LARGE_CHUNK; j >>= 1)
                hipLaunchKernelGGL(large_cx_kernel, dim3(prcnn_divup(Ntot / 2, 256), B), dim3(256), 0, s, large_ws, Ntot, j, k);
            hipLaunchKernelGGL(large_local_merge_kernel, dim3(nchunks, B), dim3(1024), lds, s, large_ws, Ntot, k);
        }
        hipLaunchKernelGGL(large_split_kernel, dim3(B), dim3(1024), 0, s, P, large_ws, Ntot);
        PRCNN_LAUNCH_CHECK(op);
        return PRCNN_OK;
    }
    P.Npad = pow2_at_least(P.N, 16);
    const int threads = max(64, ((P.Npad >> 4) + 63) / 64 * 64);
    const size_t lds = lds_sort_bytes(P.Npad) + 40 * sizeof(unsigned);
    static PrcnnLdsLimit attr_set;
    if (!attr_set.raise((const void*)sort_split_kernel, LDS_BUDGET))
        return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", op);
    hipLaunchKernelGGL(sort_split_kernel, dim3(B), dim3(threads), lds, s, P);
    PRCNN_LAUNCH_CHECK(op);
    return PRCNN_OK;
}

template <int KIND>
static int launch_greedy_nms_kind(const char* op, const NmsParams& P, int B, hipStream_t s) {
    const size_t lds = greedy_nms_lds_bytes<KIND>(max(P.post1, P.post2));
    if (lds > LDS_BUDGET)
        return prcnn_fail(PRCNN_EUNSUPPORTED, "%s: keeping up to %d boxes needs %zu B of LDS (> %d); use prcnn_nms", op,
                          max(P.post1, P.post2), lds, LDS_BUDGET);
    static PrcnnLdsLimit attr_set;
    if (!attr_set.raise((const void*)greedy_nms_kernel<KIND>, LDS_BUDGET))
        return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", op);
    hipLaunchKernelGGL(greedy_nms_kernel<KIND>, dim3(P.nseg, B), dim3(NMS_THREADS), lds, s, P);
    PRCNN_LAUNCH_CHECK(op);
    return PRCNN_OK;
}
static int launch_greedy_nms(const char* op, int kind, const NmsParams& P, int B, hipStream_t s) {
    if (kind == PRCNN_NMS_ROTATED) {
        // the prefiltered kernel where its batch fits beside the kept list (it always does for the proposal layer's 70 / 30 and the
        // detection select's 100); PRCNN_NMS_PREFILTER=0 is the A/B switch (same keep lists)
        const size_t lds = greedy_nms_rot_lds_bytes(max(P.post1, P.post2));
        if (sw_enabled(SW_NMS_PREFILTER) && lds <= LDS_BUDGET) {
            static PrcnnLdsLimit attr_set;
            if (!attr_set.raise((const void*)greedy_nms_rot_kernel, LDS_BUDGET))
                return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", op);
            hipLaunchKernelGGL(greedy_nms_rot_kernel, dim3(P.nseg, B), dim3(NMS_RT), lds, s, P);
            PRCNN_LAUNCH_CHECK(op);
            return PRCNN_OK;
        }
        return launch_greedy_nms_kind<PRCNN_NMS_ROTATED>(op, P, B, s);
    }
    {
        const size_t lds = greedy_nms_pre_lds_bytes(max(P.post1, P.post2));
        if (sw_enabled(SW_NMS_PREFILTER) && lds <= LDS_BUDGET) {
            static PrcnnLdsLimit attr_set;
            if (!attr_set.raise((const void*)greedy_nms_pre_kernel, LDS_BUDGET))
                return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", op);
            hipLaunchKernelGGL(greedy_nms_pre_kernel, dim3(P.nseg, B), dim3(NMS_RT), lds, s, P);
            PRCNN_LAUNCH_CHECK(op);
            return PRCNN_OK;
        }
    }
    return launch_greedy_nms_kind<PRCNN_NMS_NORMAL>(op, P, B, s);
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

PRCNN_API size_t prcnn_proposal_workspace_bytes(int B, int N, int pre_max, int post_max) {
    if (B <= 0) return 0;
    return align256((size_t)B * 2 * (size_t)max(pre_max, 1) * 4) + align256((size_t)B * 2 * 4) +
           align256((size_t)B * 2 * (size_t)max(post_max, 1) * 4) + align256((size_t)B * 2 * 4) + align256(large_sort_bytes(B, N));
}

PRCNN_API int prcnn_proposal_layer(const float* scores, const float* boxes3d, int B, int N, int use_range, float r0, float r1,
                                   float r2, int pre1, int pre2, int post1, int post2, float nms_thresh, int nms_kind,
                                   float* out_boxes, float* out_scores, int32_t* out_count, void* workspace,
                                   size_t workspace_bytes, prcnn_stream_t stream) {
    const char* op = "prcnn_proposal_layer";
    PRCNN_REQUIRE(B >= 0 && N >= 0, "%s: bad B=%d N=%d", op, B, N);
    PRCNN_REQUIRE(pre1 >= 0 && pre2 >= 0 && post1 >= 0 && post2 >= 0, "%s: negative top-n", op);
    PRCNN_REQUIRE(nms_kind == PRCNN_NMS_ROTATED || nms_kind == PRCNN_NMS_NORMAL, "%s: bad nms_kind %d", op, nms_kind);
    const int post = post1 + post2;
    if (B == 0 || post == 0) return PRCNN_OK;
    PRCNN_REQUIRE(out_boxes && out_scores, "%s: null output", op);
    hipStream_t s = (hipStream_t)stream;
    if (N == 0) {
        if (prcnn_fill_words(out_boxes, 0u, (size_t)B * post * 7, s) != hipSuccess ||
            prcnn_fill_words(out_scores, 0u, (size_t)B * post, s) != hipSuccess ||
            (out_count && prcnn_fill_words(out_count, 0u, (size_t)B, s) != hipSuccess))
            return prcnn_fail(PRCNN_EHIP, "%s: memset failed", op);
        return PRCNN_OK;
    }
    PRCNN_REQUIRE(scores && boxes3d && workspace, "%s: null pointer", op);
    const int pre_max = max(pre1, pre2), post_max = max(post1, post2);
    PRCNN_REQUIRE(workspace_bytes >= prcnn_proposal_workspace_bytes(B, N, pre_max, post_max), "%s: workspace %zu < %zu bytes", op,
                  workspace_bytes, prcnn_proposal_workspace_bytes(B, N, pre_max, post_max));
    PRCNN_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", op);
    char* w = (char*)workspace;
    int32_t* cand = (int32_t*)w; w += align256((size_t)B * 2 * (size_t)max(pre_max, 1) * 4);
    int32_t* cnt = (int32_t*)w; w += align256((size_t)B * 2 * 4);
    int32_t* kept = (int32_t*)w; w += align256((size_t)B * 2 * (size_t)max(post_max, 1) * 4);
    int32_t* kept_cnt = (int32_t*)w; w += align256((size_t)B * 2 * 4);
    u64* large_ws = (u64*)w;                      // only touched when N > 16384
    SortParams S;
    S.scores = scores; S.boxes3d = boxes3d; S.valid = nullptr; S.cand = cand; S.cnt = cnt;
    S.N = N; S.mode = use_range ? SPLIT_RANGE : SPLIT_ALL; S.nseg = 2; S.cand_ld = max(pre_max, 1);
    S.pre1 = pre1; S.pre2 = use_range ? pre2 : 0; S.r0 = r0; S.r1 = r1; S.r2 = r2;
    int rc = launch_sort_split(op, S, B, s, large_ws);
    if (rc) return rc;
    NmsParams Q;
    Q.boxes3d = boxes3d; Q.cand = cand; Q.cnt = cnt; Q.kept = kept; Q.kept_cnt = kept_cnt;
    Q.N = N; Q.nseg = 2; Q.cand_ld = S.cand_ld; Q.kept_ld = max(post_max, 1); Q.post1 = post1; Q.post2 = post2; Q.thresh = nms_thresh;
    rc = launch_greedy_nms(op, nms_kind, Q, B, s);
    if (rc) return rc;
    AssembleParams A;
    A.scores = scores; A.boxes3d = boxes3d; A.kept = kept; A.kept_cnt = kept_cnt; A.out_boxes = out_boxes; A.out_scores = out_scores;
    A.out_count = out_count; A.N = N; A.kept_ld = Q.kept_ld; A.post = post;
    hipLaunchKernelGGL(assemble_kernel, dim3(B), dim3(128), 0, s, A);
    PRCNN_LAUNCH_CHECK(op);
    return PRCNN_OK;
}

PRCNN_API size_t prcnn_nms_batched_workspace_bytes(int B, int M) {
    if (B <= 0 || M <= 0) return 0;
    return align256((size_t)B * M * 4) + align256((size_t)B * 4) + align256(large_sort_bytes(B, M));
}

PRCNN_API int prcnn_nms_batched(const float* boxes3d, const float* scores, const uint8_t* valid, int B, int M, float thresh, int kind,
                                int max_keep, int32_t* keep, int32_t* num_keep, void* workspace, size_t workspace_bytes,
                                prcnn_stream_t stream) {
    const char* op = "prcnn_nms_batched";
    PRCNN_REQUIRE(B >= 0 && M >= 0 && max_keep >= 0, "%s: bad B=%d M=%d max_keep=%d", op, B, M, max_keep);
    PRCNN_REQUIRE(kind == PRCNN_NMS_ROTATED || kind == PRCNN_NMS_NORMAL, "%s: bad kind %d", op, kind);
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(num_keep, "%s: null num_keep", op);
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {
        if (prcnn_fill_words(num_keep, 0u, (size_t)B, s) != hipSuccess) return prcnn_fail(PRCNN_EHIP, "%s: memset failed", op);
        return PRCNN_OK;
    }
    if (max_keep == 0 || max_keep > M) max_keep = M;
    PRCNN_REQUIRE(boxes3d && scores && keep && workspace, "%s: null pointer", op);
    PRCNN_REQUIRE(workspace_bytes >= prcnn_nms_batched_workspace_bytes(B, M), "%s: workspace %zu < %zu bytes", op, workspace_bytes,
                  prcnn_nms_batched_workspace_bytes(B, M));
    char* w = (char*)workspace;
    int32_t* cand = (int32_t*)w; w += align256((size_t)B * M * 4);
    int32_t* cnt = (int32_t*)w; w += align256((size_t)B * 4);
    u64* large_ws = (u64*)w;
    SortParams S;
    S.scores = scores; S.boxes3d = boxes3d; S.valid = valid; S.cand = cand; S.cnt = cnt;
    S.N = M; S.mode = valid ? SPLIT_VALID : SPLIT_ALL; S.nseg = 1; S.cand_ld = M; S.pre1 = M; S.pre2 = 0; S.r0 = S.r1 = S.r2 = 0.f;
    int rc = launch_sort_split(op, S, B, s, large_ws);
    if (rc) return rc;
    NmsParams Q;
    Q.boxes3d = boxes3d; Q.cand = cand; Q.cnt = cnt; Q.kept = keep; Q.kept_cnt = num_keep;
    Q.N = M; Q.nseg = 1; Q.cand_ld = M; Q.kept_ld = max_keep; Q.post1 = max_keep; Q.post2 = 0; Q.thresh = thresh;
    return launch_greedy_nms(op, kind, Q, B, s);
}
