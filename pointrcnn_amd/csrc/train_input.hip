// train_input.hip -- the GT-augmentation side of the RPN training input on the device (BASELINE config 4,
// `train_rcnn.py --train_mode rpn` on tools/cfgs/default.yaml, GT_AUG_ENABLED).
//
//   prcnn_corner_iou3d  : kitti_utils.get_iou3d (lib/utils/kitti_utils.py:195-235) on two corner sets, one thread per pair;
//                         the arithmetic is quad_clip.h (fp32 heights, exact double clip in place of shapely).
//   prcnn_gt_aug_sample : the sampling loop of KittiRCNNDataset.apply_gt_aug_to_one_scene (kitti_rcnn_dataset.py:414-497)
//                         plus the apply-probability draw of get_rpn_sample (:279), one 64-lane workgroup per frame.  The tries
//                         are sequential (each one depends on what was accepted before); inside a try the collision list is
//                         tested one lane per box, with the list in LDS.  Most pairs are decided by a conservative fp32
//                         separating-axis test (an axis that separates the two bottoms by more than the rounding margin proves
//                         that the exact clip is empty, so the IoU is exactly 0); the rest go to the double clip.  No atomics:
//                         the result depends on (seed, frame, inputs) only, never on the launch geometry.
//
// Randomness (counter_rand.h, shared with scene.hip, whose header lists every stream id): r(stream, frame, position);
// u01(r) = fp32(r >> 8) * 2^-24 widened to double, below(r, n) = (r * n) >> 32:
//   stream 30, position 0   np.random.rand() < GT_AUG_APPLY_PROB                  (get_rpn_sample, kitti_rcnn_dataset.py:279)
//   stream 31, position 0   extra_gt_num = randint(10, GT_EXTRA_NUM) = 10 + below(r, GT_EXTRA_NUM - 10)   (:419-420)
//   stream 32, position t   try t: p = rand(), easy list iff p > GT_AUG_HARD_RATIO                      (:437-439)
//   stream 33, position t   try t: index = randint(0, len(list)) = below(r, len(list))                    (:441-448)
// t counts every try that was started (0-based), skipped ones included.
#include "common.h"
#include "quad_clip.h"
#include "counter_rand.h"

constexpr int GTA_THREADS = 64;
constexpr int GTA_LIST_CAP = 256;         // collision list entries (scene boxes + accepted objects) held in LDS
constexpr int GTA_MAX_ACCEPT = 64;

__device__ __forceinline__ double ti_u01(unsigned r) { return (double)((float)(r >> 8) * (1.0f / 16777216.0f)); }
__device__ __forceinline__ unsigned ti_below(unsigned r, unsigned n) { return (unsigned)(((uint64_t)r * n) >> 32); }

// ------------------------------------------------------------------------------------------------ corner_iou3d
__global__ void corner_iou3d_kernel(const float* __restrict__ a, int N, const float* __restrict__ b, int M, float* __restrict__ iou3d,
                                    float* __restrict__ bev) {
    const size_t total = (size_t)N * M;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const float* ca = a + (p / M) * 24;
        const float* cb = b + (p % M) * 24;
        float lo_a, hi_a, lo_b, hi_b;
        qc_heights(ca, lo_a, hi_a);
        qc_heights(cb, lo_b, hi_b);
        const float h = qc_h_overlap(lo_a, hi_a, lo_b, hi_b);
        float v3 = 0.0f, vb = 0.0f;
        if (h != 0.0f) {
            const QcQuad qa = qc_make(ca), qb = qc_make(cb);
            qc_ratios(qa, qb, h, hi_a - lo_a, hi_b - lo_b, v3, vb);
        }
        iou3d[p] = v3;
        if (bev) bev[p] = vb;
    }
}

PRCNN_API int prcnn_corner_iou3d(const float* corners_a, int N, const float* corners_b, int M, float* iou3d, float* iou_bev,
                                 prcnn_stream_t stream) {
    PRCNN_REQUIRE(N >= 0 && M >= 0, "prcnn_corner_iou3d: bad shape N=%d M=%d", N, M);
    if (N == 0 || M == 0) return PRCNN_OK;
    PRCNN_REQUIRE(corners_a && corners_b && iou3d, "prcnn_corner_iou3d: null pointer");
    const size_t total = (size_t)N * M;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(corner_iou3d_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, corners_a, N, corners_b, M, iou3d, iou_bev);
    PRCNN_LAUNCH_CHECK("prcnn_corner_iou3d");
    return PRCNN_OK;
}

// ------------------------------------------------------------------------------------------------ gt_aug_sample
struct GtAugParams {
    const float* gt;            // (B, G, 7) collision boxes of every frame (non-DontCare labels)
    const int32_t* num_gt;      // (B) or NULL
    const double* planes;       // (B, 4) road planes a b c d, normalised
    const float* db_boxes;      // (D, 7)
    const float* db_alpha;      // (D)
    const int32_t* db_npts;     // (D)
    const int32_t* easy;        // (E) database ids of the easy list (hard_ratio > 0)
    const int32_t* hard;        // (H)
    int B, G, D, E, H, K, tries;
    int extra_num, rand_num;
    double apply_prob, hard_ratio;
    double scope[6];
    int use_scope;
    unsigned seed;
    int32_t* count;             // (B)
    int32_t* db_id;             // (B, K)
    float* boxes;               // (B, K, 7)
    float* alpha;               // (B, K)
    double* y_shift;            // (B, K)
    int32_t* stats;             // (B, 4) applied, extra_gt_num, counted tries, tries started
    int32_t* status;            // (B)
};

// the (8,3) corners of one box as kitti_utils.boxes3d_to_corners3d forms them in fp32: local corners
// x = +-l/2, z = +-w/2, y = 0 / -h; rotated by a (8,3) x (3,3) product accumulated left to right from 0; then shifted
__device__ __forceinline__ void ti_corners(const float* bx, float* c) {
    const float h = bx[3], w = bx[4], l = bx[5];
    const float cs = cosf(bx[6]), sn = sinf(bx[6]), nsn = -sn;
    const float hl = l / 2.0f, hw = w / 2.0f;
    const float xs[8] = {hl, hl, -hl, -hl, hl, hl, -hl, -hl};
    const float zs[8] = {hw, -hw, -hw, hw, hw, -hw, -hw, hw};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float ys = k < 4 ? 0.0f : -h;
        const float xr = (xs[k] * cs + ys * 0.0f) + zs[k] * sn;
        const float yr = (xs[k] * 0.0f + ys * 1.0f) + zs[k] * 0.0f;
        const float zr = (xs[k] * nsn + ys * 0.0f) + zs[k] * cs;
        c[3 * k + 0] = bx[0] + xr;
        c[3 * k + 1] = bx[1] + yr;
        c[3 * k + 2] = bx[2] + zr;
    }
}

struct GtaList {
    float x[GTA_LIST_CAP][4], z[GTA_LIST_CAP][4];
    float lo[GTA_LIST_CAP], hi[GTA_LIST_CAP];
};

__device__ __forceinline__ void gta_store(GtaList& L, int i, const float* c) {
    for (int k = 0; k < 4; ++k) {
        L.x[i][k] = c[3 * k];
        L.z[i][k] = c[3 * k + 2];
    }
    qc_heights(c, L.lo[i], L.hi[i]);
}

// true when an axis (an edge normal of either bottom quad) separates the two bottoms by more than a bound on the fp32 rounding of
// the projections: then the exact regions are disjoint with a positive gap and the double clip returns exactly 0
__device__ __forceinline__ bool gta_separated(const float* ax, const float* az, const float* bx, const float* bz) {
    float S = 1.0f;
    for (int k = 0; k < 4; ++k) S = fmaxf(S, fmaxf(fmaxf(fabsf(ax[k]), fabsf(az[k])), fmaxf(fabsf(bx[k]), fabsf(bz[k]))));
    for (int e = 0; e < 8; ++e) {
        const float* ex = e < 4 ? ax : bx;
        const float* ez = e < 4 ? az : bz;
        const int i = e & 3, j = (i + 1) & 3;
        const float nx = -(ez[j] - ez[i]), nz = ex[j] - ex[i];
        const float margin = 1e-5f * (fabsf(nx) + fabsf(nz)) * S;
        float amin = INFINITY, amax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
        for (int k = 0; k < 4; ++k) {
            const float pa = ax[k] * nx + az[k] * nz, pb = bx[k] * nx + bz[k] * nz;
            amin = fminf(amin, pa); amax = fmaxf(amax, pa);
            bmin = fminf(bmin, pb); bmax = fmaxf(bmax, pb);
        }
        if (amax < bmin - margin || bmax < amin - margin) return true;
    }
    return false;
}

// iou3d(new, entry) >= 1e-8 (fp32 compare, as numpy compares the fp32 IoU array with the Python float)
__device__ bool gta_collides(const GtaList& L, int i, const float* nc, float nlo, float nhi) {
    const float h = qc_h_overlap(nlo, nhi, L.lo[i], L.hi[i]);
    if (h == 0.0f) return false;
    float ax[4], az[4];
    for (int k = 0; k < 4; ++k) { ax[k] = nc[3 * k]; az[k] = nc[3 * k + 2]; }
    if (gta_separated(ax, az, L.x[i], L.z[i])) return false;
    float eb[24];
    for (int k = 0; k < 4; ++k) { eb[3 * k] = L.x[i][k]; eb[3 * k + 1] = 0.0f; eb[3 * k + 2] = L.z[i][k]; }
    const QcQuad qa = qc_make(nc), qb = qc_make(eb);
    float v3, vb;
    qc_ratios(qa, qb, h, nhi - nlo, L.hi[i] - L.lo[i], v3, vb);
    return !(v3 < 1e-8f);
}

__global__ __launch_bounds__(GTA_THREADS) void gt_aug_sample_kernel(GtAugParams P) {
    __shared__ GtaList L;
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned seed = P.seed;
    const int ng = P.num_gt ? min(max(P.num_gt[b], 0), P.G) : P.G;
    for (int i = tid; i < ng; i += GTA_THREADS) {           // the scene's boxes, w and l + 0.5 (:423-426)
        const float* g = P.gt + ((size_t)b * P.G + i) * 7;
        float bx[7] = {g[0], g[1], g[2], g[3], g[4] + 0.5f, g[5] + 0.5f, g[6]};
        float c[24];
        ti_corners(bx, c);
        gta_store(L, i, c);
    }
    __syncthreads();
    const double pa = P.planes[b * 4 + 0], pb = P.planes[b * 4 + 1], pc = P.planes[b * 4 + 2], pd = P.planes[b * 4 + 3];
    int st = 0, acc = 0, cnt = 0, started = 0, extra = P.extra_num;
    const int applied = ti_u01(scene_rand(seed, 30, b, 0)) < P.apply_prob;
    if (applied && P.rand_num) {
        if (P.extra_num <= 10) st = 1;                       // np.random.randint(10, n <= 10) raises
        else extra = 10 + (int)ti_below(scene_rand(seed, 31, b, 0), (unsigned)(P.extra_num - 10));
    }
    if (applied && st == 0) {
        for (int t = 0; t < P.tries; ++t) {
            if (cnt > extra) break;
            started = t + 1;
            int id;
            if (P.hard_ratio > 0.0) {
                const bool easy = ti_u01(scene_rand(seed, 32, b, t)) > P.hard_ratio;
                const int n = easy ? P.E : P.H;
                if (n <= 0) { st = 1; break; }               // randint(0, 0) raises
                const unsigned k = ti_below(scene_rand(seed, 33, b, t), (unsigned)n);
                id = easy ? P.easy[k] : P.hard[k];
            } else {
                if (P.D <= 0) { st = 1; break; }
                id = (int)ti_below(scene_rand(seed, 33, b, t), (unsigned)P.D);
            }
            if (id < 0 || id >= P.D) { st = 3; break; }      // an easy / hard list that does not belong to this database
            const float* db = P.db_boxes + (size_t)id * 7;
            if (P.use_scope) {                               // check_pc_range on the centre before the move (:451-452)
                const double x = db[0], y = db[1], z = db[2];
                if (!(P.scope[0] <= x && x <= P.scope[1] && P.scope[2] <= y && y <= P.scope[3] && P.scope[4] <= z && z <= P.scope[5]))
                    continue;
            }
            if (P.db_npts[id] < 5) continue;                 // :454-455
            const double cur_h = ((-pd - pa * (double)db[0]) - pc * (double)db[2]) / pb;   // :458-460, in double
            const double move = (double)db[1] - cur_h;
            const float ny = (float)((double)db[1] - move);
            float eb[7] = {db[0], ny, db[2], db[3], db[4] + 0.5f, db[5] + 0.5f, db[6]};
            ++cnt;
            const int n = ng + acc;
            if (n == 0) { st = 1; break; }                   // iou3d.max() of an empty array raises
            float nc[24];
            ti_corners(eb, nc);
            float nlo, nhi;
            qc_heights(nc, nlo, nhi);
            int hit = 0;
            for (int i = tid; i < n && !hit; i += GTA_THREADS) hit = gta_collides(L, i, nc, nlo, nhi);
            if (__syncthreads_or(hit)) continue;
            if (acc >= P.K || n >= GTA_LIST_CAP) { st = 2; break; }
            if (tid == 0) {
                gta_store(L, n, nc);
                const size_t o = (size_t)b * P.K + acc;
                P.db_id[o] = id;
                for (int q = 0; q < 7; ++q) P.boxes[o * 7 + q] = q == 1 ? ny : db[q];
                P.alpha[o] = P.db_alpha[id];
                P.y_shift[o] = move;
            }
            ++acc;
            __syncthreads();
        }
    }
    for (int j = acc + tid; j < P.K; j += GTA_THREADS) {
        const size_t o = (size_t)b * P.K + j;
        P.db_id[o] = -1;
        for (int q = 0; q < 7; ++q) P.boxes[o * 7 + q] = 0.0f;
        P.alpha[o] = 0.0f;
        P.y_shift[o] = 0.0;
    }
    if (tid == 0) {
        P.count[b] = acc;
        P.stats[b * 4 + 0] = applied;
        P.stats[b * 4 + 1] = extra;
        P.stats[b * 4 + 2] = cnt;
        P.stats[b * 4 + 3] = started;
        P.status[b] = st;
    }
}

PRCNN_API int prcnn_gt_aug_sample(const float* gt_boxes3d, const int32_t* num_gt, const double* planes, int B, int G,
                                  const float* db_boxes, const float* db_alpha, const int32_t* db_npts, int D, const int32_t* easy_idx,
                                  int E, const int32_t* hard_idx, int H, const double* cfg4, const double* scope, int try_times, int K,
                                  uint32_t seed, int32_t* count, int32_t* db_id, float* boxes3d, float* alpha, double* y_shift,
                                  int32_t* stats, int32_t* status, prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && G >= 0 && D >= 0 && E >= 0 && H >= 0, "prcnn_gt_aug_sample: bad shape B=%d G=%d D=%d E=%d H=%d", B, G, D, E, H);
    PRCNN_REQUIRE(K >= 1 && K <= GTA_MAX_ACCEPT, "prcnn_gt_aug_sample: K=%d (1..%d accepted objects per frame)", K, GTA_MAX_ACCEPT);
    PRCNN_REQUIRE(G + K <= GTA_LIST_CAP, "prcnn_gt_aug_sample: G + K = %d > %d (the collision list is LDS-resident)", G + K, GTA_LIST_CAP);
    PRCNN_REQUIRE(try_times >= 0 && try_times <= 100000, "prcnn_gt_aug_sample: try_times=%d", try_times);
    PRCNN_REQUIRE(cfg4, "prcnn_gt_aug_sample: null cfg4");
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(planes && db_boxes && db_alpha && db_npts && count && db_id && boxes3d && alpha && y_shift && stats && status,
                  "prcnn_gt_aug_sample: null pointer");
    PRCNN_REQUIRE(G == 0 || gt_boxes3d, "prcnn_gt_aug_sample: null gt_boxes3d");
    const double hard_ratio = cfg4[3];
    PRCNN_REQUIRE(hard_ratio <= 0.0 || ((E == 0 || easy_idx) && (H == 0 || hard_idx)), "prcnn_gt_aug_sample: null easy / hard list");
    GtAugParams P = {};
    P.gt = gt_boxes3d; P.num_gt = num_gt; P.planes = planes;
    P.db_boxes = db_boxes; P.db_alpha = db_alpha; P.db_npts = db_npts; P.easy = easy_idx; P.hard = hard_idx;
    P.B = B; P.G = G; P.D = D; P.E = E; P.H = H; P.K = K; P.tries = try_times;
    P.extra_num = (int)cfg4[0]; P.rand_num = cfg4[1] != 0.0; P.apply_prob = cfg4[2]; P.hard_ratio = hard_ratio;
    P.use_scope = scope != nullptr;
    for (int q = 0; q < 6; ++q) P.scope[q] = scope ? scope[q] : 0.0;
    P.seed = seed;
    P.count = count; P.db_id = db_id; P.boxes = boxes3d; P.alpha = alpha; P.y_shift = y_shift; P.stats = stats; P.status = status;
    hipLaunchKernelGGL(gt_aug_sample_kernel, dim3(B), dim3(GTA_THREADS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_gt_aug_sample");
    return PRCNN_OK;
}
