// aug_scene.hip -- the offline GT-augmented scenes (the `train_aug` split) on the device: tools/generate_aug_scene.py for a batch of
// frames.  Step 1 of the reference's offline RCNN recipe; its host loop makes, per frame, up to 50 boxes_iou3d_gpu calls with a blocking
// .cpu() each and one whole-scan pts_in_boxes3d_cpu per accepted object.
//
//   prcnn_aug_scene_sample : AugSceneGenerator.aug_one_scene's sampling loop (:157-219), one 64-lane workgroup per frame, no host round
//                            trip.  The tries are sequential; inside a try the collision list (LDS: the raw boxes and their RBox) is
//                            tested one lane per entry with iou3d_pair_s (the arithmetic of prcnn_boxes_iou3d), the clip's point list
//                            in a lane-private LDS column.  The per-try arithmetic and the list of differences from the online loop of
//                            train_input.hip are aug_scene_math.h.  No atomics: the result depends on (seed, frame id, inputs) only.
//   prcnn_aug_scene_count / _fill : aug_one_epoch_scene :240-248 + aug_one_scene :205-231: lidar -> rect and the valid flag
//                            (scene_project), every valid point inside an accepted box with h + 2 dropped (make_box + pt_in_box<true>,
//                            the test of prcnn_pts_in_boxes3d), the survivors in raw order, then the accepted objects' database points
//                            in acceptance order with y - y_shift.  The output size depends on the data: as in gt_database.hip a count
//                            pass gives the rows of every frame, the caller allocates, a fill pass writes.
//       augs_tile_kernel<false> : one 1024-thread block per (1024-point tile, frame): survivors of the tile -> (frame, tile) table
//       augs_scan_kernel        : one wave per frame: exclusive prefix of the tile counts, the survivors, the frame's rows
//       augs_tile_kernel<true>  : the tiles recomputed; a survivor's row = frame offset + tile prefix + waves before + lanes below
//       augs_paste_kernel       : one block per (accepted object, frame): its database points behind the survivors
//     Positions come from prefix sums only, never from an atomic append (there is no counter to clear): two runs write the same bytes.
//     Every row is checked against [0, total_out) and against the frame's own range before it is written.
// A frame with status 1 or count 0 keeps its valid cloud unchanged.
#include "scene_common.h"
#include "box_test.h"
#include "iou3d_pair.h"
#include "aug_scene_math.h"

constexpr int AUGS_THREADS = 64;
constexpr int AUGS_LIST_CAP = 256;          // collision list entries (labels + accepted objects) held in LDS
constexpr int AUGS_MAX_K = 64;
constexpr int AUGS_TILE = 1024;
constexpr int AUGS_TILE_WAVES = AUGS_TILE / 64;

// ------------------------------------------------------------------------------------------------ sampler
struct AugsSampleParams {
    const float* gt;            // (B, G, 7) non-DontCare labels
    const int32_t* num_gt;      // (B) or NULL
    const double* planes;       // (B, 4)
    const int32_t* frame_ids;   // (B) the key of the random table: the new sample id
    const float* db_boxes;      // (D, 7)
    const int32_t* db_npts;     // (D)
    int B, G, D, K;
    double scope[6];
    unsigned seed;
    int32_t* count;             // (B)
    int32_t* db_id;             // (B, K)
    float* boxes;               // (B, K, 7) placed, unenlarged
    double* y_shift;            // (B, K)
    int32_t* stats;             // (B, 3) extra_gt_num, cnt, tries spent
    int32_t* status;            // (B)
};

__device__ __forceinline__ void augs_list_put(float (*raw)[7], RBox* rb, int i, const float* box) {
    float e[7], bev[5];
    augs_enlarge(box, e);
    for (int q = 0; q < 7; ++q) raw[i][q] = e[q];
    bev_of(e, bev);
    make_rbox(bev, rb[i]);
}

__global__ __launch_bounds__(AUGS_THREADS) void augs_sample_kernel(AugsSampleParams P) {
    __shared__ float s_raw[AUGS_LIST_CAP][7];
    __shared__ RBox s_rb[AUGS_LIST_CAP];
    __shared__ float s_clip[CLIP_LDS_FLOATS * AUGS_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const unsigned seed = P.seed, frame = (unsigned)P.frame_ids[b];
    const int ng = P.num_gt ? min(max(P.num_gt[b], 0), P.G) : P.G;
    for (int i = tid; i < ng; i += AUGS_THREADS) augs_list_put(s_raw, s_rb, i, P.gt + ((size_t)b * P.G + i) * 7);
    __syncthreads();
    double plane[4];
    for (int q = 0; q < 4; ++q) plane[q] = P.planes[b * 4 + q];
    ClipLds clip;
    clip.b = s_clip + tid;
    clip.T = AUGS_THREADS;
    const int extra = augs_extra_num(seed, frame);
    int st = 0, acc = 0, cnt = 0, spent = 0;
    for (int t = 0; t < AUGS_TRIES; ++t) {
        spent = t + 1;
        if (P.D <= 1) { st = 1; break; }                       // randint(0, D - 1) raises
        const int id = augs_draw_index(seed, frame, t, P.D);
        const float* db = P.db_boxes + (size_t)id * 7;
        if (!augs_in_scope(db, P.scope)) continue;
        if (cnt > extra) break;
        if (P.db_npts[id] < 5) continue;
        double move;
        const float ny = augs_plane_move(db, plane, move);
        const float nb[7] = {db[0], ny, db[2], db[3], db[4], db[5], db[6]};
        ++cnt;
        const int n = ng + acc;
        if (n == 0) { st = 1; break; }                         // max() of an empty IoU array raises
        int hit = 0;
        for (int i = tid; i < n && !hit; i += AUGS_THREADS) hit = augs_collides(iou3d_pair_s(nb, s_raw[i], s_rb[i], clip));
        if (__syncthreads_or(hit)) continue;
        if (acc >= P.K || acc >= AUGS_MAX_ACCEPT || n >= AUGS_LIST_CAP) { st = 2; break; }
        if (tid == 0) {
            augs_list_put(s_raw, s_rb, n, nb);
            const size_t o = (size_t)b * P.K + acc;
            P.db_id[o] = id;
            for (int q = 0; q < 7; ++q) P.boxes[o * 7 + q] = nb[q];
            P.y_shift[o] = move;
        }
        ++acc;
        __syncthreads();
    }
    for (int j = acc + tid; j < P.K; j += AUGS_THREADS) {
        const size_t o = (size_t)b * P.K + j;
        P.db_id[o] = -1;
        for (int q = 0; q < 7; ++q) P.boxes[o * 7 + q] = 0.0f;
        P.y_shift[o] = 0.0;
    }
    if (tid == 0) {
        P.count[b] = acc;
        P.stats[b * 3 + 0] = extra;
        P.stats[b * 3 + 1] = cnt;
        P.stats[b * 3 + 2] = spent;
        P.status[b] = st;
    }
}

PRCNN_API int prcnn_aug_scene_sample(const float* gt_boxes3d, const int32_t* num_gt, const double* planes, const int32_t* frame_ids, int B,
                                     int G, const float* db_boxes, const int32_t* db_npts, int D, const double* scope, int K, uint32_t seed,
                                     int32_t* count, int32_t* db_id, float* boxes3d, double* y_shift, int32_t* stats, int32_t* status,
                                     prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && G >= 0 && D >= 0, "prcnn_aug_scene_sample: bad shape B=%d G=%d D=%d", B, G, D);
    PRCNN_REQUIRE(K >= AUGS_MAX_ACCEPT && K <= AUGS_MAX_K, "prcnn_aug_scene_sample: K=%d (%d..%d: a frame accepts up to %d objects)", K,
                  AUGS_MAX_ACCEPT, AUGS_MAX_K, AUGS_MAX_ACCEPT);
    PRCNN_REQUIRE(G + AUGS_MAX_ACCEPT <= AUGS_LIST_CAP, "prcnn_aug_scene_sample: G + %d = %d > %d (the collision list is LDS-resident)",
                  AUGS_MAX_ACCEPT, G + AUGS_MAX_ACCEPT, AUGS_LIST_CAP);
    PRCNN_REQUIRE(scope, "prcnn_aug_scene_sample: null scope (the tool always crops by PC_AREA_SCOPE)");
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(planes && frame_ids && count && db_id && boxes3d && y_shift && stats && status, "prcnn_aug_scene_sample: null pointer");
    PRCNN_REQUIRE((G == 0 || gt_boxes3d) && (D == 0 || (db_boxes && db_npts)), "prcnn_aug_scene_sample: null boxes");
    AugsSampleParams P = {};
    P.gt = gt_boxes3d; P.num_gt = num_gt; P.planes = planes; P.frame_ids = frame_ids; P.db_boxes = db_boxes; P.db_npts = db_npts;
    P.B = B; P.G = G; P.D = D; P.K = K; P.seed = seed;
    for (int q = 0; q < 6; ++q) P.scope[q] = scope[q];
    P.count = count; P.db_id = db_id; P.boxes = boxes3d; P.y_shift = y_shift; P.stats = stats; P.status = status;
    hipLaunchKernelGGL(augs_sample_kernel, dim3(B), dim3(AUGS_THREADS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_aug_scene_sample");
    return PRCNN_OK;
}

// ------------------------------------------------------------------------------------------------ cloud builder
struct AugsBuildParams {
    const float4* raw;          // (total, 4) x y z intensity, lidar frame
    const int64_t* off;         // (B+1)
    const float* calib;         // (B, 24)
    const int32_t* img_hw;      // (B, 2)
    double scope[6];
    int use_scope;
    int64_t total;
    int B, T, K, D;             // T tiles of AUGS_TILE points cover max_points_per_frame
    const int32_t* acc_count;   // (B)
    const int32_t* acc_id;      // (B, K)
    const float* acc_boxes;     // (B, K, 7)
    const double* acc_shift;    // (B, K)
    const int32_t* acc_status;  // (B)
    const float* db_points;     // (db_total, 3)
    const float* db_inten;      // (db_total)
    const int64_t* db_off;      // (D+1)
    int64_t db_total;
    int32_t* tile_cnt;          // (B, T) survivors of a tile
    int32_t* tile_off;          // (B, T) their exclusive prefix
    int32_t* kept;              // (B) survivors of the frame
    int32_t* rows;              // (B) survivors + pasted points          -- count pass
    const int64_t* out_off;     // (B+1)                                  -- fill pass
    int64_t total_out;
    float4* out;                // (total_out, 4)
    int32_t* src;               // (total_out) raw index of a survivor, -1 - database row of a pasted point
};

__device__ __forceinline__ int augs_frame_points(const AugsBuildParams& P, int b, int64_t& o) {
    o = P.off[b];
    int64_t n64 = P.off[b + 1] - o;
    if (o < 0 || n64 < 0 || o + n64 > P.total) n64 = 0;
    const int64_t cover = (int64_t)P.T * AUGS_TILE;
    return (int)(n64 < cover ? n64 : cover);
}

// the accepted objects a frame pastes: none when the reference raised on it
__device__ __forceinline__ int augs_frame_accepted(const AugsBuildParams& P, int b) {
    return P.acc_status[b] == 1 ? 0 : min(max(P.acc_count[b], 0), P.K);
}

// the database rows of accepted object k of frame b: -> how many, first row in o; none for an id or a range outside the database
__device__ __forceinline__ int augs_object_points(const AugsBuildParams& P, int b, int k, int64_t& o) {
    const int id = P.acc_id[(size_t)b * P.K + k];
    o = 0;
    if (id < 0 || id >= P.D) return 0;
    o = P.db_off[id];
    const int64_t n = P.db_off[id + 1] - o;
    if (o < 0 || n < 0 || o + n > P.db_total || n >= (1LL << 30)) return 0;
    return (int)n;
}

template <bool FILL>
__global__ __launch_bounds__(AUGS_TILE) void augs_tile_kernel(AugsBuildParams P) {
    __shared__ BoxConst sbox[AUGS_MAX_K];
    __shared__ int wcnt[AUGS_TILE_WAVES];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t o;
    const int n = augs_frame_points(P, b, o);
    if ((int64_t)t * AUGS_TILE >= n) {
        if (!FILL && tid == 0) P.tile_cnt[(size_t)b * P.T + t] = 0;
        return;
    }
    const int k = augs_frame_accepted(P, b);
    if (tid < k) {
        const float* bx = P.acc_boxes + ((size_t)b * P.K + tid) * 7;
        float big[7];
        for (int c = 0; c < 7; c++) big[c] = bx[c];
        big[3] = bx[3] + 2.0f;                                 // :205-206, a float32 add
        sbox[tid] = make_box(big);
    }
    __syncthreads();
    const int i = t * AUGS_TILE + tid;
    bool keep = false;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    RectPoint r = {0.f, 0.f, 0.f, false};
    if (i < n) {
        p = P.raw[o + i];
        r = scene_project(p, P.calib + b * 24, P.img_hw[b * 2], P.img_hw[b * 2 + 1], P.scope, P.use_scope);
        keep = r.valid;
        for (int q = 0; q < k && keep; q++) keep = !pt_in_box<true>(sbox[q], r.x, r.y, r.z);
    }
    const unsigned long long bv = __ballot(keep);
    if (lane == 0) wcnt[wave] = (int)__popcll(bv);
    __syncthreads();
    if (!FILL) {
        if (tid == 0) {
            int c = 0;
            for (int w = 0; w < AUGS_TILE_WAVES; w++) c += wcnt[w];
            P.tile_cnt[(size_t)b * P.T + t] = c;
        }
        return;
    }
    if (keep) {
        int before = 0;
        for (int w = 0; w < wave; w++) before += wcnt[w];
        const int64_t lo = P.out_off[b], hi = P.out_off[b + 1];
        const int64_t pos = lo + P.tile_off[(size_t)b * P.T + t] + before + (int)__popcll(bv & ((1ULL << lane) - 1ULL));
        if (pos >= 0 && pos >= lo && pos < hi && pos < P.total_out) {
            P.out[pos] = make_float4(r.x, r.y, r.z, p.w);
            P.src[pos] = i;
        }
    }
}

__global__ __launch_bounds__(64) void augs_scan_kernel(AugsBuildParams P) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const size_t row = (size_t)b * P.T;
    int carry = 0;
    for (int t0 = 0; t0 < P.T; t0 += 64) {
        const int t = t0 + lane;
        const int v = t < P.T ? P.tile_cnt[row + t] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(incl, d);
            if (lane >= d) incl += u;
        }
        if (t < P.T) P.tile_off[row + t] = carry + incl - v;
        carry += __shfl(incl, 63);
    }
    if (lane == 0) {
        int64_t pasted = 0, o;
        const int k = augs_frame_accepted(P, b);
        for (int q = 0; q < k; q++) pasted += augs_object_points(P, b, q, o);
        P.kept[b] = carry;
        const int64_t rows = (int64_t)carry + pasted;
        P.rows[b] = rows < (1LL << 31) - 1 ? (int32_t)rows : -1;       // -1: the frame's rows do not fit the int32 count
    }
}

__global__ __launch_bounds__(256) void augs_paste_kernel(AugsBuildParams P) {
    const int b = blockIdx.y, k = blockIdx.x;
    if (k >= augs_frame_accepted(P, b)) return;
    int64_t o, skip;
    int64_t before = P.kept[b];
    for (int q = 0; q < k; q++) before += augs_object_points(P, b, q, skip);
    const int n = augs_object_points(P, b, k, o);
    const double move = P.acc_shift[(size_t)b * P.K + k];
    const int64_t lo = P.out_off[b], hi = P.out_off[b + 1];
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const int64_t pos = lo + before + j;
        if (pos >= 0 && pos >= lo && pos < hi && pos < P.total_out) {
            const float* q3 = P.db_points + (o + j) * 3;
            P.out[pos] = make_float4(q3[0], augs_point_y(q3[1], move), q3[2], P.db_inten[o + j]);
            P.src[pos] = (int32_t)(-1 - (o + j));
        }
    }
}

static size_t augs_table_bytes(int64_t max_points_per_frame, int B) {
    const size_t T = (size_t)((max_points_per_frame + AUGS_TILE - 1) / AUGS_TILE);
    return (((size_t)B * T * sizeof(int32_t) + 63) / 64) * 64;
}

PRCNN_API size_t prcnn_aug_scene_workspace_bytes(int64_t max_points_per_frame, int B) {
    if (max_points_per_frame < 0 || B < 0) return 0;
    return 2 * augs_table_bytes(max_points_per_frame, B) + (((size_t)B * sizeof(int32_t) + 63) / 64) * 64 + 64;
}

// what both entry points require of the arguments they share; fills P
static int augs_common(const char* who, AugsBuildParams& P, const float* raw, const int64_t* offsets, int B, int64_t total_points,
                       int max_points_per_frame, const float* calib, const int32_t* img_hw, const double* scope, const int32_t* acc_count,
                       const int32_t* acc_db_id, const float* acc_boxes3d, const int32_t* acc_status, int K, const int64_t* db_offsets, int D,
                       int64_t db_total_points, void* workspace, size_t workspace_bytes) {
    PRCNN_REQUIRE(B <= 65535 && D >= 0 && db_total_points >= 0 && db_total_points < (1LL << 31), "%s: bad shape B=%d D=%d db points=%ld", who, B,
                  D, (long)db_total_points);
    PRCNN_REQUIRE(K >= 1 && K <= AUGS_MAX_K, "%s: K=%d (1..%d accepted objects per frame: their constants are LDS-resident)", who, K, AUGS_MAX_K);
    const int rc = scene_check_frames(who, raw, offsets, B, total_points, max_points_per_frame, calib, 0, AUGS_TILE);
    if (rc != PRCNN_OK || B == 0) return rc;
    PRCNN_REQUIRE(img_hw && acc_count && acc_db_id && acc_boxes3d && acc_status && db_offsets, "%s: null pointer", who);
    PRCNN_REQUIRE(workspace && ((uintptr_t)workspace % 4) == 0 && workspace_bytes >= prcnn_aug_scene_workspace_bytes(max_points_per_frame, B),
                  "%s: workspace too small", who);
    P.raw = reinterpret_cast<const float4*>(raw); P.off = offsets; P.calib = calib; P.img_hw = img_hw;
    P.use_scope = scope != nullptr;
    for (int q = 0; q < 6; q++) P.scope[q] = scope ? scope[q] : 0.0;
    P.total = total_points; P.B = B; P.T = prcnn_divup(max_points_per_frame, AUGS_TILE); P.K = K; P.D = D;
    P.acc_count = acc_count; P.acc_id = acc_db_id; P.acc_boxes = acc_boxes3d; P.acc_status = acc_status;
    P.db_off = db_offsets; P.db_total = db_total_points;
    char* w = static_cast<char*>(workspace);
    const size_t tb = augs_table_bytes(max_points_per_frame, B);
    P.tile_cnt = reinterpret_cast<int32_t*>(w);
    P.tile_off = reinterpret_cast<int32_t*>(w + tb);
    P.kept = reinterpret_cast<int32_t*>(w + 2 * tb);
    return PRCNN_OK;
}

PRCNN_API int prcnn_aug_scene_count(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                    const float* calib, const int32_t* img_hw, const double* scope, const int32_t* acc_count,
                                    const int32_t* acc_db_id, const float* acc_boxes3d, const int32_t* acc_status, int K,
                                    const int64_t* db_offsets, int D, int64_t db_total_points, int32_t* rows, void* workspace,
                                    size_t workspace_bytes, prcnn_stream_t stream) {
    AugsBuildParams P = {};
    const int rc = augs_common("prcnn_aug_scene_count", P, raw, offsets, B, total_points, max_points_per_frame, calib, img_hw, scope, acc_count,
                               acc_db_id, acc_boxes3d, acc_status, K, db_offsets, D, db_total_points, workspace, workspace_bytes);
    if (rc != PRCNN_OK || B == 0) return rc;
    PRCNN_REQUIRE(rows, "prcnn_aug_scene_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    P.rows = rows;
    if (P.T > 0) {
        hipLaunchKernelGGL(augs_tile_kernel<false>, dim3(P.T, B), dim3(AUGS_TILE), 0, s, P);
        PRCNN_LAUNCH_CHECK("prcnn_aug_scene_count(count)");
    }
    hipLaunchKernelGGL(augs_scan_kernel, dim3(B), dim3(64), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_aug_scene_count(scan)");
    return PRCNN_OK;
}

PRCNN_API int prcnn_aug_scene_fill(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                   const float* calib, const int32_t* img_hw, const double* scope, const int32_t* acc_count,
                                   const int32_t* acc_db_id, const float* acc_boxes3d, const double* acc_y_shift, const int32_t* acc_status,
                                   int K, const float* db_points, const float* db_intensity, const int64_t* db_offsets, int D,
                                   int64_t db_total_points, const int64_t* out_offsets, int64_t total_out, float* out, int32_t* src,
                                   void* workspace, size_t workspace_bytes, prcnn_stream_t stream) {
    AugsBuildParams P = {};
    const int rc = augs_common("prcnn_aug_scene_fill", P, raw, offsets, B, total_points, max_points_per_frame, calib, img_hw, scope, acc_count,
                               acc_db_id, acc_boxes3d, acc_status, K, db_offsets, D, db_total_points, workspace, workspace_bytes);
    if (rc != PRCNN_OK || B == 0) return rc;
    PRCNN_REQUIRE(total_out >= 0, "prcnn_aug_scene_fill: total_out=%ld", (long)total_out);
    if (total_out == 0) return PRCNN_OK;
    PRCNN_REQUIRE(acc_y_shift && out_offsets && out && src && (db_total_points == 0 || (db_points && db_intensity)),
                  "prcnn_aug_scene_fill: null pointer");
    PRCNN_REQUIRE(((uintptr_t)out % 16) == 0, "prcnn_aug_scene_fill: out must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    P.acc_shift = acc_y_shift; P.db_points = db_points; P.db_inten = db_intensity;
    P.out_off = out_offsets; P.total_out = total_out; P.out = reinterpret_cast<float4*>(out); P.src = src;
    if (P.T > 0) {
        hipLaunchKernelGGL(augs_tile_kernel<true>, dim3(P.T, B), dim3(AUGS_TILE), 0, s, P);
        PRCNN_LAUNCH_CHECK("prcnn_aug_scene_fill(survivors)");
    }
    hipLaunchKernelGGL(augs_paste_kernel, dim3(K, B), dim3(256), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_aug_scene_fill(paste)");
    return PRCNN_OK;
}
