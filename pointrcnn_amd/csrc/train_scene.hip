// train_scene.hip -- the RPN TRAINING batch on the device: KittiRCNNDataset.get_rpn_sample in TRAIN mode
// (lib/datasets/kitti_rcnn_dataset.py:246-362, RPN.FIXED false) for a whole batch, from raw scans to augmented points and boxes.
// The sampling loop of the GT augmentation runs before it (train_input.hip, prcnn_gt_aug_sample), the label kernel after it
// (roipool3d.hip, prcnn_rpn_labels); this file is everything between the two:
//
//   1. valid points          lidar -> rect, get_valid_flag: scene_project of scene_common.h, arithmetic contract of scene.hip.
//   2. GT augmentation       every valid scene point inside an accepted object's box with h + 2 is dropped (:484-490, the test of
//                            gt_aug_edit_kernel); the accepted objects' database points are added with y' = fp32(double(y) - y_shift)
//                            (:470).  Pasted points pass no image or scope test.  Frames whose sampler status is 1 or 3 are built
//                            without paste or removal.
//   3. the npoints draw      over the EDITED cloud (:285-301), rule and status codes of scene_sample_kernel.  A candidate's identity
//                            (the i of r(stream, frame, i), streams 0, 1, 2) is the raw index for a scene point and
//                            n_raw + j for the j-th pasted point, counted in accepted order, then database point order.
//   4. label boxes           the caller's training labels (filtrate_objects, host code), then the accepted objects' placed boxes (:324-331).
//   5. data_augmentation     stage 1, mustaug False (:513-570).  Random values: streams 34 (aug_enable[i] = 1 - u01(r), position i),
//                            35 (angle = lo + (hi - lo) * u01(r)), 36 (scale, the same form) -- listed in scene.hip's header.
//                            Rotation: c = cos(angle), s = sin(angle) in double; x' = fp32(double(x) * c + double(z) * (-s)),
//                            z' = fp32(double(x) * s + double(z) * c) for points and box centres; beta = atan2f(z', x') (ref_trig.h),
//                            ry' = ((sign(beta) * fp32(pi)) / 2 + alpha) - beta in fp32.  Scaling: fp32(v * fp32(scale)) for points
//                            and box columns 0..5.  Flip: x = -x, ry = sign(ry) * fp32(pi) - ry.  Individually rounded, no contraction.
//
//   tscene_box_kernel    : one workgroup per frame: draws the frame's augmentation (reported through `aug`, which the sample pass
//                          reads back), builds the (G + K)-row augmented gt_boxes3d.
//   tscene_flag_kernel   : scene_flag_kernel with the accepted-box test (<= 64 BoxConst in LDS) between scene_project and
//                          scene_append: removed points never enter the candidate list.
//   tscene_paste_kernel  : one workgroup per (accepted object, frame): appends the object's points to the same list with their
//                          far bit and draw key (one atomic per object).
//   tscene_sample_kernel : npoints <= 16384.  One workgroup per frame: scene_select_sort; the row writer reads the raw scan
//                          (scene_rect) or the database (applying y_shift) and applies step 5 as it writes.
//   16384 < npoints <= 65536 (prcnn_train_scene_prepare_large) replaces the sample launch as scene.hip does:
//   tscene_select_large_kernel (the draw into the frame's HBM key array), scene_large_shuffle (scene.hip's three sort kernels),
//   tscene_rows_kernel (one thread per output row, the same row writer).
// The frame head of the params, the projection, the append, the draw and the host prelude are scene_common.h's.
// No (N + P) cloud is materialised and nothing synchronises with the host between the launches.  The selected set and the output
// order depend on (seed, frame, identity) only, never on the order in which the atomics append.
#include "common.h"
#include "scene_common.h"
#include "box_test.h"

constexpr int TS_MAX_ACCEPT = 64;
constexpr int TS_MAX_BOXES = 128;          // G + K: what prcnn_rpn_labels takes per frame
constexpr int TS_PASTE_THREADS = 256;
constexpr float TS_PI = 3.14159274101257324f;      // fp32(np.pi)

struct TrainSceneParams : SceneFrames {      // list: frame b at off[b] + b * K * db_max; out_src: raw index, or n_raw + j (pasted)
    const float* gt;            // (B, G, 7) training labels
    const float* gt_alpha;      // (B, G)
    const int32_t* num_gt;      // (B) or NULL
    int G;
    const int32_t* acc_count;   // (B) prcnn_gt_aug_sample's outputs; NULL: no GT augmentation
    const int32_t* acc_id;      // (B, K)
    const float* acc_boxes;     // (B, K, 7)
    const float* acc_alpha;     // (B, K)
    const double* acc_shift;    // (B, K)
    const int32_t* acc_status;  // (B)
    int K;
    const float* db_pts;        // (P, 3)
    const float* db_int;        // (P)
    const int64_t* db_off;      // (D+1)
    int D, db_max;
    int methods;                // bit 0 rotation, 1 scaling, 2 flip in AUG_METHOD_LIST
    double prob[3], rot_lo, rot_hi, sc_lo, sc_hi;
    float* out_input;           // (B, npoints, 4) or NULL
    float* out_feat;            // (B, npoints)
    float* out_gt;              // (B, G + K, 7)
    int32_t* out_num_gt;        // (B)
    double* aug;                // (B, 8) enable[3], angle, cos, sin, scale, flip
};

// accepted objects that are pasted into frame b: none when the sampler left the reference's domain (status 1, 3)
__device__ __forceinline__ int ts_accepted(const TrainSceneParams& P, int b) {
    if (!P.acc_count) return 0;
    const int st = P.acc_status[b];
    if (st == 1 || st == 3) return 0;
    return min(max(P.acc_count[b], 0), P.K);
}

// points of accepted object a of frame b: first database row through `first`; 0 for an id outside the database
__device__ __forceinline__ int ts_object_points(const TrainSceneParams& P, int b, int a, int64_t& first) {
    const int id = P.acc_id[(size_t)b * P.K + a];
    first = 0;
    if (id < 0 || id >= P.D) return 0;
    first = P.db_off[id];
    const int64_t m = P.db_off[id + 1] - first;
    return (int)min(max(m, (int64_t)0), (int64_t)P.db_max);
}

__device__ __forceinline__ uint2* ts_list(const TrainSceneParams& P, int b) {
    return P.list + P.off[b] + (int64_t)b * P.K * P.db_max;
}

__device__ __forceinline__ float ts_sign(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : v); }      // np.sign: 0 -> 0, nan -> nan

__global__ __launch_bounds__(TS_MAX_BOXES) void tscene_box_kernel(TrainSceneParams P) {
    __shared__ double sa[8];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        double e[3];
        for (int i = 0; i < 3; ++i) e[i] = 1.0 - scene_u01(scene_rand(P.seed, 34u, (unsigned)b, (unsigned)i));
        double angle = NAN, c = NAN, s = NAN, scale = NAN, flip = 0.0;
        if ((P.methods & 1) && e[0] < P.prob[0]) {
            angle = P.rot_lo + (P.rot_hi - P.rot_lo) * scene_u01(scene_rand(P.seed, 35u, (unsigned)b, 0u));
            c = cos(angle);
            s = sin(angle);
        }
        if ((P.methods & 2) && e[1] < P.prob[1]) scale = P.sc_lo + (P.sc_hi - P.sc_lo) * scene_u01(scene_rand(P.seed, 36u, (unsigned)b, 0u));
        if ((P.methods & 4) && e[2] < P.prob[2]) flip = 1.0;
        sa[0] = e[0]; sa[1] = e[1]; sa[2] = e[2]; sa[3] = angle; sa[4] = c; sa[5] = s; sa[6] = scale; sa[7] = flip;
        for (int q = 0; q < 8; ++q) P.aug[(size_t)b * 8 + q] = sa[q];
    }
    __syncthreads();
    const int ng = P.num_gt ? min(max(P.num_gt[b], 0), P.G) : P.G;
    const int na = ts_accepted(P, b);
    if (tid == 0) P.out_num_gt[b] = ng + na;
    const int rows = P.G + P.K;
    if (tid >= rows) return;
    float r[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float alpha = 0.f;
    const bool live = tid < ng + na;
    if (tid < ng) {
        const float* g = P.gt + ((size_t)b * P.G + tid) * 7;
        for (int q = 0; q < 7; ++q) r[q] = g[q];
        alpha = P.gt_alpha[(size_t)b * P.G + tid];
    } else if (live) {
        const size_t o = (size_t)b * P.K + (tid - ng);
        for (int q = 0; q < 7; ++q) r[q] = P.acc_boxes[o * 7 + q];
        alpha = P.acc_alpha[o];
    }
    if (live) {
        if (sa[3] == sa[3]) {                                   // rotation (:526-537)
            const double c = sa[4], s = sa[5], x = (double)r[0], z = (double)r[2];
            const float nx = (float)(x * c + z * (-s)), nz = (float)(x * s + z * c);
            r[0] = nx; r[2] = nz;
            const float beta = prcnn_ref_atan2f(nz, nx);
            r[6] = ((ts_sign(beta) * TS_PI) / 2.0f + alpha) - beta;
        }
        if (sa[6] == sa[6]) {                                   // scaling (:548-551)
            const float fs = (float)sa[6];
            for (int q = 0; q < 6; ++q) r[q] = r[q] * fs;
        }
        if (sa[7] != 0.0) {                                     // flip (:554-560)
            r[0] = -r[0];
            r[6] = ts_sign(r[6]) * TS_PI - r[6];
        }
    }
    float* o = P.out_gt + ((size_t)b * rows + tid) * 7;
    for (int q = 0; q < 7; ++q) o[q] = r[q];
}

__global__ __launch_bounds__(SCENE_THREADS) void tscene_flag_kernel(TrainSceneParams P) {
    __shared__ BoxConst sbox[TS_MAX_ACCEPT];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t o = P.off[b];
    const int n = (int)(P.off[b + 1] - o);
    if ((int64_t)blockIdx.x * SCENE_THREADS >= n) return;
    const int na = ts_accepted(P, b);
    if (tid < na) {
        const float* bx = P.acc_boxes + ((size_t)b * P.K + tid) * 7;
        float big[7];
#pragma unroll
        for (int c = 0; c < 7; c++) big[c] = bx[c];
        big[3] = bx[3] + 2.0f;                                 // kitti_rcnn_dataset.py:484-485 (float32 add, as numpy does it)
        sbox[tid] = make_box(big);
    }
    __syncthreads();
    const int i = blockIdx.x * SCENE_THREADS + tid;
    bool valid = false, far = false;
    if (i < n) {
        const RectPoint r = scene_project(P.raw[o + i], P.calib + b * 24, P.img_hw[b * 2], P.img_hw[b * 2 + 1], P.scope, P.use_scope);
        valid = r.valid;
        if (valid) {
            bool inside = false;
            for (int q = 0; q < na; q++) inside |= pt_in_box(sbox[q], r.x, r.y, r.z);
            valid = !inside;
        }
        far = valid && !(r.z < 40.0f);                         // kitti_rcnn_dataset.py:288: near = depth < 40.0
    }
    scene_append(valid, far, i, ts_list(P, b), P.counters + b * 2, P.seed, b);
}

__global__ __launch_bounds__(TS_PASTE_THREADS) void tscene_paste_kernel(TrainSceneParams P) {
    __shared__ int base, nfar;
    const int a = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (a >= ts_accepted(P, b)) return;
    int64_t first;
    const int m = ts_object_points(P, b, a, first);
    if (m == 0) return;
    unsigned ident0 = (unsigned)(P.off[b + 1] - P.off[b]);      // n_raw + the points of the objects accepted before this one
    for (int q = 0; q < a; ++q) {
        int64_t f0;
        ident0 += (unsigned)ts_object_points(P, b, q, f0);
    }
    if (tid == 0) { base = atomicAdd(P.counters + b * 2, m); nfar = 0; }
    __syncthreads();
    uint2* L = ts_list(P, b) + base;
    int far_here = 0;
    for (int j = tid; j < m; j += TS_PASTE_THREADS) {
        const bool far = !(P.db_pts[(first + j) * 3 + 2] < 40.0f);
        const unsigned key = scene_rand(P.seed, 0u, (unsigned)b, ident0 + (unsigned)j) >> 2;
        L[j] = make_uint2(key | (far ? SCENE_FAR : 0u), ident0 + (unsigned)j);
        far_here += far ? 1 : 0;
    }
    if (far_here) atomicAdd(&nfar, far_here);
    __syncthreads();
    if (tid == 0 && nfar > 0) atomicAdd(P.counters + b * 2 + 1, nfar);
}

// where the pasted identities of a frame live: filled by one thread (ts_paste_fill), read by the row writer after a barrier
struct TsPaste {
    unsigned base[TS_MAX_ACCEPT + 1];         // identity (minus n_raw) of every accepted object's first point
    int64_t first[TS_MAX_ACCEPT];             // its first database row
    double shift[TS_MAX_ACCEPT];
};
__device__ __forceinline__ void ts_paste_fill(const TrainSceneParams& P, int b, int na, TsPaste& T) {
    unsigned run = 0;
    for (int a = 0; a < na; ++a) {
        int64_t first;
        const int m = ts_object_points(P, b, a, first);
        T.base[a] = run; T.first[a] = first; T.shift[a] = P.acc_shift[(size_t)b * P.K + a];
        run += (unsigned)m;
    }
    T.base[na] = run;
}

// the frame's augmentation as tscene_box_kernel reported it
struct TsAug {
    bool rot, scl, flip;
    double rc, rs;
    float fs;
};
__device__ __forceinline__ TsAug ts_load_aug(const TrainSceneParams& P, int b) {
    const double* A = P.aug + (size_t)b * 8;
    TsAug g;
    g.rot = A[3] == A[3]; g.scl = A[6] == A[6]; g.flip = A[7] != 0.0;
    g.rc = A[4]; g.rs = A[5]; g.fs = (float)A[6];
    return g;
}

// output row j of frame b is the candidate with identity i: a raw point (i < n_raw) or a pasted one, augmented as it is written
__device__ __forceinline__ void ts_write_row(const TrainSceneParams& P, int b, int j, unsigned i, int na, const TsPaste& T, const TsAug& g) {
    const int np = P.npoints;
    const int64_t o = P.off[b];
    const unsigned n_raw = (unsigned)(P.off[b + 1] - o);
    float* oxyz = P.out_xyz + (size_t)b * np * 3;
    float* oin = P.out_input ? P.out_input + (size_t)b * np * 4 : nullptr;
    float x, y, z, w;
    if (i < n_raw) {
        const float4 p = P.raw[o + i];
        scene_rect(p, P.calib + b * 24, x, y, z);
        w = p.w;
    } else {
        const unsigned jj = i - n_raw;
        int a = 0;
        while (a + 1 < na && jj >= T.base[a + 1]) ++a;
        const int64_t q = T.first[a] + (jj - T.base[a]);
        x = P.db_pts[q * 3];
        y = (float)((double)P.db_pts[q * 3 + 1] - T.shift[a]);    // new_gt_points[:, 1] -= move_height (:470)
        z = P.db_pts[q * 3 + 2];
        w = P.db_int[q];
    }
    if (g.rot) {
        const double dx = (double)x, dz = (double)z;
        x = (float)(dx * g.rc + dz * (-g.rs));
        z = (float)(dx * g.rs + dz * g.rc);
    }
    if (g.scl) { x = x * g.fs; y = y * g.fs; z = z * g.fs; }
    if (g.flip) x = -x;
    const float feat = w - 0.5f;
    oxyz[j * 3 + 0] = x; oxyz[j * 3 + 1] = y; oxyz[j * 3 + 2] = z;
    if (oin) { oin[j * 4 + 0] = x; oin[j * 4 + 1] = y; oin[j * 4 + 2] = z; oin[j * 4 + 3] = feat; }
    P.out_feat[(size_t)b * np + j] = feat;
    P.out_src[(size_t)b * np + j] = (int32_t)i;
}

__global__ __launch_bounds__(SCENE_THREADS) void tscene_sample_kernel(TrainSceneParams P) {
    extern __shared__ u64 keys[];
    __shared__ SceneLds lds;
    __shared__ TsPaste paste;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = P.counters[b * 2], f = P.counters[b * 2 + 1];
    const int np = P.npoints;
    const int na = ts_accepted(P, b);
    if (tid == 0) {
        P.nvalid[b] = n;
        ts_paste_fill(P, b, na, paste);                         // ordered before the row writer by scene_select_sort's barriers
    }
    if (n == 0) {
        scene_empty_frame(P, b, P.out_feat, P.out_input);
        return;
    }
    const SceneSel ss = scene_select_sort(ts_list(P, b), n, f, np, P.NP, P.seed, (unsigned)b, keys, lds);
    const int total = ss.total;                                 // == npoints unless the status is 1
    // ---- rows in shuffled order (a short selection -- status 1 -- repeats cyclically), augmented as they are written
    const TsAug g = ts_load_aug(P, b);
    for (int j = tid; j < np; j += SCENE_THREADS) ts_write_row(P, b, j, (unsigned)keys[lds_phys(j < total ? j : j % total)], na, paste, g);
    if (tid == 0) P.status[b] = ss.status;
}

// ---- 16384 < npoints <= 65536: select -> scene_large_shuffle -> rows (scene.hip's header) ------------------------------------------
__global__ __launch_bounds__(SCENE_THREADS) void tscene_select_large_kernel(TrainSceneParams P) {
    __shared__ SceneLds lds;
    const int b = blockIdx.x;
    scene_select_large(P, b, ts_list(P, b), P.out_feat, P.out_input, lds);
}

// grid (ceil(npoints / SCENE_THREADS), B): one thread per output row
__global__ __launch_bounds__(SCENE_THREADS) void tscene_rows_kernel(TrainSceneParams P) {
    __shared__ TsPaste paste;
    const int b = blockIdx.y, j = blockIdx.x * SCENE_THREADS + threadIdx.x;
    const int total = P.large_total[b];
    if (total == 0) return;                                     // block-uniform: the whole frame was written by the select launch
    const int na = ts_accepted(P, b);
    if (threadIdx.x == 0) ts_paste_fill(P, b, na, paste);
    __syncthreads();
    if (j >= P.npoints) return;
    ts_write_row(P, b, j, scene_large_identity(P, b, j, total), na, paste, ts_load_aug(P, b));
}

PRCNN_API size_t prcnn_train_scene_workspace_bytes(int64_t total_points, int B, int K, int db_max_points) {
    if (total_points < 0 || B < 0 || K < 0 || db_max_points < 0) return 0;
    const size_t entries = (size_t)total_points + (size_t)B * K * db_max_points;     // frame b holds n_raw[b] + K * db_max_points
    return entries * sizeof(uint2) + scene_list_offset(B) + 64;
}

// both exports; max_npoints = the export's domain
static int train_scene_prepare_any(const char* who, int max_npoints, const float* raw, const int64_t* offsets, int B, int64_t total_points,
                                   int max_points_per_frame, const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                                        const float* gt_boxes3d, const float* gt_alpha, const int32_t* num_gt, int G,
                                        const int32_t* acc_count, const int32_t* acc_db_id, const float* acc_boxes3d, const float* acc_alpha,
                                        const double* acc_y_shift, const int32_t* acc_status, int K, const float* db_points,
                                        const float* db_intensity, const int64_t* db_offsets, int D, int db_max_points,
                                        const double* aug_cfg, float* out_xyz, float* out_input, float* out_features, int32_t* out_src,
                                        int32_t* nvalid, int32_t* status, float* out_gt_boxes3d, int32_t* out_num_gt, double* aug,
                                        void* workspace, size_t workspace_bytes, prcnn_stream_t stream) {
    if (max_npoints == SCENE_SMALL_MAX)
        PRCNN_REQUIRE(npoints > 0 && npoints <= 16384, "%s: npoints=%d (1..16384: the shuffle is one LDS-resident sort per frame)", who, npoints);
    else
        PRCNN_REQUIRE(npoints > 0 && npoints <= SCENE_LARGE_MAX, "%s: npoints=%d (1..65536: the shuffle sorts at most four 16384-key chunks per frame)", who, npoints);
    const bool large = npoints > SCENE_SMALL_MAX;
    PRCNN_REQUIRE(G >= 0 && K >= 0 && K <= TS_MAX_ACCEPT, "%s: G=%d K=%d (K: 0..%d accepted objects per frame)", who, G, K, TS_MAX_ACCEPT);
    PRCNN_REQUIRE(G + K <= TS_MAX_BOXES, "%s: G + K = %d > %d (what prcnn_rpn_labels takes per frame)", who, G + K, TS_MAX_BOXES);
    PRCNN_REQUIRE(D >= 0 && db_max_points >= 0, "%s: bad database shape D=%d max=%d", who, D, db_max_points);
    PRCNN_REQUIRE(aug_cfg, "%s: null aug_cfg", who);
    const bool paste = acc_count != nullptr && K > 0;
    const int Kp = paste ? K : 0;
    int rc = scene_check_frames(who, raw, offsets, B, total_points, max_points_per_frame, calib, (long)Kp * db_max_points, SCENE_THREADS);
    if (rc != PRCNN_OK || B == 0) return rc;
    PRCNN_REQUIRE(img_hw && out_xyz && out_features && out_src && nvalid && status && out_num_gt && aug,
                  "%s: null pointer", who);
    PRCNN_REQUIRE(G + K == 0 || out_gt_boxes3d, "%s: null out_gt_boxes3d", who);
    PRCNN_REQUIRE(G == 0 || (gt_boxes3d && gt_alpha), "%s: null gt_boxes3d / gt_alpha", who);
    PRCNN_REQUIRE(!paste || (acc_db_id && acc_boxes3d && acc_alpha && acc_y_shift && acc_status && db_offsets &&
                             (db_max_points == 0 || (db_points && db_intensity))),
                  "%s: the accepted objects need db_id, boxes3d, alpha, y_shift, status and the database", who);
    const size_t small_bytes = prcnn_train_scene_workspace_bytes(total_points, B, Kp, db_max_points);
    PRCNN_REQUIRE(workspace && workspace_bytes >= scene_large_bytes(small_bytes, B, npoints), "%s: workspace too small", who);
    PRCNN_REQUIRE(!large || ((uintptr_t)workspace % 8) == 0, "%s: workspace must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    TrainSceneParams P = {};
    scene_fill_frames(P, raw, offsets, B, calib, img_hw, scope, npoints, seed, workspace, out_xyz, out_src, nvalid, status);
    if (large) scene_fill_large(P, workspace, small_bytes);
    P.gt = gt_boxes3d; P.gt_alpha = gt_alpha; P.num_gt = num_gt; P.G = G;
    P.acc_count = paste ? acc_count : nullptr; P.acc_id = acc_db_id; P.acc_boxes = acc_boxes3d; P.acc_alpha = acc_alpha;
    P.acc_shift = acc_y_shift; P.acc_status = acc_status; P.K = K;
    P.db_pts = db_points; P.db_int = db_intensity; P.db_off = db_offsets; P.D = D; P.db_max = paste ? db_max_points : 0;
    P.methods = (aug_cfg[0] != 0.0 ? 1 : 0) | (aug_cfg[1] != 0.0 ? 2 : 0) | (aug_cfg[2] != 0.0 ? 4 : 0);
    for (int q = 0; q < 3; q++) P.prob[q] = aug_cfg[3 + q];
    P.rot_lo = aug_cfg[6]; P.rot_hi = aug_cfg[7]; P.sc_lo = aug_cfg[8]; P.sc_hi = aug_cfg[9];
    P.out_input = out_input; P.out_feat = out_features; P.out_gt = out_gt_boxes3d; P.out_num_gt = out_num_gt; P.aug = aug;
    if ((rc = scene_reset_counters(who, P, s)) != PRCNN_OK) return rc;
    hipLaunchKernelGGL(tscene_box_kernel, dim3(B), dim3(TS_MAX_BOXES), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_train_scene_prepare(boxes)");
    if (max_points_per_frame > 0) {
        hipLaunchKernelGGL(tscene_flag_kernel, dim3(prcnn_divup(max_points_per_frame, SCENE_THREADS), B), dim3(SCENE_THREADS), 0, s, P);
        PRCNN_LAUNCH_CHECK("prcnn_train_scene_prepare(flags)");
    }
    if (paste && db_max_points > 0) {
        hipLaunchKernelGGL(tscene_paste_kernel, dim3(K, B), dim3(TS_PASTE_THREADS), 0, s, P);
        PRCNN_LAUNCH_CHECK("prcnn_train_scene_prepare(paste)");
    }
    if (!large) return scene_launch_sample<tscene_sample_kernel>(who, P, s);
    hipLaunchKernelGGL(tscene_select_large_kernel, dim3(B), dim3(SCENE_THREADS), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_train_scene_prepare_large(select)");
    if ((rc = scene_large_shuffle(who, P, s)) != PRCNN_OK) return rc;
    hipLaunchKernelGGL(tscene_rows_kernel, dim3(prcnn_divup(npoints, SCENE_THREADS), B), dim3(SCENE_THREADS), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_train_scene_prepare_large(rows)");
    return PRCNN_OK;
}

// the argument list both exports share (include/prcnn_pointops.h states it in full)
#define TS_ARGS_DECL                                                                                                                                  \
    const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame, const float* calib, const int32_t* img_hw,       \
        const double* scope, int npoints, uint32_t seed, const float* gt_boxes3d, const float* gt_alpha, const int32_t* num_gt, int G,                \
        const int32_t* acc_count, const int32_t* acc_db_id, const float* acc_boxes3d, const float* acc_alpha, const double* acc_y_shift,              \
        const int32_t* acc_status, int K, const float* db_points, const float* db_intensity, const int64_t* db_offsets, int D,                        \
        int db_max_points, const double* aug_cfg, float* out_xyz, float* out_input, float* out_features, int32_t* out_src, int32_t* nvalid,           \
        int32_t* status, float* out_gt_boxes3d, int32_t* out_num_gt, double* aug, void* workspace, size_t workspace_bytes, prcnn_stream_t stream
#define TS_ARGS                                                                                                                              \
    raw, offsets, B, total_points, max_points_per_frame, calib, img_hw, scope, npoints, seed, gt_boxes3d, gt_alpha, num_gt, G, acc_count,     \
        acc_db_id, acc_boxes3d, acc_alpha, acc_y_shift, acc_status, K, db_points, db_intensity, db_offsets, D, db_max_points, aug_cfg, out_xyz, \
        out_input, out_features, out_src, nvalid, status, out_gt_boxes3d, out_num_gt, aug, workspace, workspace_bytes, stream

PRCNN_API int prcnn_train_scene_prepare(TS_ARGS_DECL) { return train_scene_prepare_any("prcnn_train_scene_prepare", SCENE_SMALL_MAX, TS_ARGS); }

PRCNN_API size_t prcnn_train_scene_large_workspace_bytes(int64_t total_points, int B, int K, int db_max_points, int npoints) {
    if (total_points < 0 || B < 0 || K < 0 || db_max_points < 0 || npoints < 0) return 0;
    return scene_large_bytes(prcnn_train_scene_workspace_bytes(total_points, B, K, db_max_points), B, npoints);
}

PRCNN_API int prcnn_train_scene_prepare_large(TS_ARGS_DECL) {
    return train_scene_prepare_any("prcnn_train_scene_prepare_large", SCENE_LARGE_MAX, TS_ARGS);
}
