// scene.hip -- the RPN input builder on the device: raw velodyne scans -> the (B, npoints, 3)
// rect-camera clouds the backbone consumes, for a whole batch in two launches and with no host round trip.
//
// Replaces lib/datasets/kitti_rcnn_dataset.py:246-310 (get_rpn_sample, inference branch), which does per frame, in numpy on
// one dataloader core: lidar_to_rect (calibration.py:51-59), rect_to_img (:61-70), get_valid_flag (image bounds, depth >= 0,
// PC_AREA_SCOPE; kitti_rcnn_dataset.py:198-219), boolean-mask compaction, then the npoints sampling of :285-306 -- every
// point at depth >= 40 m kept, the rest drawn without replacement, the result shuffled; scans with fewer valid points
// than npoints are topped up with a draw without replacement from themselves.
//
// Arithmetic contract (shared with oracle/prcnn_oracle.c, canonical like the other ops): fp32, individually rounded,
// left to right, no FMA:  rect_c = ((x*M[0][c] + y*M[1][c]) + z*M[2][c]) + M[3][c]   with M = V2C^T . R0^T formed by the
// host in fp32 exactly as calibration.py:57 does;  hom_r = ((rx*P[r][0] + ry*P[r][1]) + rz*P[r][2]) + P[r][3];
// u = hom_0 / rz, v = hom_1 / rz (IEEE division; the reference divides by the RECT z, calibration.py:68);
// depth = hom_2 - P[2][3];  the PC_AREA_SCOPE comparisons are done in double against the double bounds, as numpy does.
// (The reference's np.dot goes through a BLAS sgemm whose summation order is unspecified: its values can differ from the
// canonical ones in the last ulp -- tests/test_oracle_scene.py pins the oracle against the reference's own output.)
//
// Randomness: numpy's global Mersenne-Twister stream cannot be reproduced by a parallel kernel (nor does the reference seed
// it); the draw is re-specified with a counter-based generator so that GPU and oracle agree bit for bit:
//   r(stream, frame, i) = mix(i ^ mix(frame * 0x9E3779B9 + mix(seed + stream * 0x85EBCA6B))),  mix = the 32-bit finaliser below;
//   "draw k of a candidate set without replacement" = the k candidates with the smallest (r(0,.) >> 2, raw index);
//   "shuffle" = ascending order of (r(1,.), raw index) (top-up copies use r(2,.)).
// Stream ids in use (each reference random call has a fixed (stream, frame, position); counter_rand.h is the generator):
//   0-2    this file (draw, shuffle, top-up shuffle; position = raw index)
//   10-13, 20   proposal_target.hip (RoI sampling and noise)
//   30     train_input.hip: get_rpn_sample's np.random.rand() < GT_AUG_APPLY_PROB (kitti_rcnn_dataset.py:279), position 0 -- u01(r)
//   31     train_input.hip: randint(10, GT_EXTRA_NUM) (:419), position 0 -- 10 + below(r, GT_EXTRA_NUM - 10)
//   32     train_input.hip: per try t, the easy / hard rand() (:437), position t -- u01(r)
//   33     train_input.hip: per try t, randint(0, len(list)) (:441-448), position t -- below(r, len)
//   34     train_scene.hip: data_augmentation's aug_enable = 1 - np.random.rand(3) (:521), position i = 0, 1, 2 -- 1 - u01(r)
//   35     train_scene.hip: angle = np.random.uniform(-pi / AUG_ROT_RANGE, pi / AUG_ROT_RANGE) (:527), position 0 -- lo + (hi - lo) * u01(r)
//   36     train_scene.hip: scale = np.random.uniform(0.95, 1.05) (:549), position 0 -- lo + (hi - lo) * u01(r)
//   40, 42, 43, 50   rcnn_offline.hip (offline RoI sampling and noise; 41 left free); 51-53 its per-RoI augmentation (enable, angle, scale)
//   60     aug_scene.hip: extra_gt_num = randint(10, 15) (tools/generate_aug_scene.py:157), position 0 -- 10 + below(r, 5)
//   61     aug_scene.hip: per try t, randint(0, D - 1) (:175), position t -- below(r, D - 1); frame = the new sample id
//   70 + ordinal   head_tail.hip: the training heads' Dropout masks (head_tail_math.h), ordinal = the nn.Dropout module's place in
//          the model's named_modules(); frame = the module's call counter, position r * K + k -- keep iff the float32 u01(r) >= p
//   with u01(r) = fp32(r >> 8) * 2^-24 widened to double, below(r, n) = (r * n) >> 32.
//   train_scene.hip also uses streams 0-2 for its own draw; there the position is the candidate's identity: the raw index
//   for a scene point, n_raw + j for the j-th pasted point.
// Both are exact uniform draws / permutations when r is uniform; the selected SET and the output ORDER depend only on
// (seed, frame, raw index), never on the order in which the kernels' atomics append.
//
//   scene_flag_kernel   : one thread per raw point: scene_project, the far flag, scene_append.
//   scene_sample_kernel : npoints <= 16384.  One workgroup per frame: scene_select_sort (draw + LDS shuffle), then the rows
//                         recomputed and written in shuffled order.
// 16384 < npoints <= 65536 (prcnn_scene_prepare_large) replaces the sample launch by a chain of plain launches on the same stream;
// launch order is the only order between them, no workgroup waits for another:
//   scene_select_large_kernel : one workgroup per frame: the same draw (scene_draw, scene_gather), the selection written unsorted
//                               to the frame's NP-entry key array in the workspace, the tail filled with ~0; nvalid, status, total.
//   scene_chunk_sort_kernel   : one workgroup per 16384-key chunk: block_sort16 in LDS, odd chunks descending.
//   scene_cx_kernel           : one compare-exchange pass of stride >= 16384 in HBM.
//   scene_chunk_merge_kernel  : strides < 16384 of one merge stage, block_merge16 per chunk.
//                               (3 launches for NP = 32768, 6 for NP = 65536 -- proposal.hip's score sort is the same network.)
//   scene_rows_kernel         : one thread per output row: the row writer of scene_sample_kernel, keys read from HBM.
// train_scene.hip launches the three sort kernels through scene_large_shuffle.
// The pieces are scene_common.h's, which every other pass over raw frames builds from too.
#include "scene_common.h"

struct SceneParams : SceneFrames {
    float* out_int;             // (B, npoints) intensity - 0.5
};

__global__ __launch_bounds__(SCENE_THREADS) void scene_flag_kernel(SceneParams P) {
    const int b = blockIdx.y;
    const int64_t o = P.off[b];
    const int n = (int)(P.off[b + 1] - o);
    if ((int64_t)blockIdx.x * SCENE_THREADS >= n) return;
    const int i = blockIdx.x * SCENE_THREADS + threadIdx.x;
    bool valid = false, far = false;
    if (i < n) {
        const RectPoint r = scene_project(P.raw[o + i], P.calib + b * 24, P.img_hw[b * 2], P.img_hw[b * 2 + 1], P.scope, P.use_scope);
        valid = r.valid;
        far = valid && !(r.z < 40.0f);                 // kitti_rcnn_dataset.py:288: near = depth < 40.0
    }
    scene_append(valid, far, i, P.list + o, P.counters + b * 2, P.seed, b);
}

// output row j of frame b (o: its first raw point) is raw point i
__device__ __forceinline__ void scene_write_row(const SceneParams& P, int b, int64_t o, int j, unsigned i) {
    const int np = P.npoints;
    float* oxyz = P.out_xyz + (size_t)b * np * 3;
    const float4 p = P.raw[o + i];
    scene_rect(p, P.calib + b * 24, oxyz[j * 3], oxyz[j * 3 + 1], oxyz[j * 3 + 2]);
    P.out_int[(size_t)b * np + j] = p.w - 0.5f;
    P.out_src[(size_t)b * np + j] = (int32_t)i;
}

__global__ __launch_bounds__(SCENE_THREADS) void scene_sample_kernel(SceneParams P) {
    extern __shared__ u64 keys[];
    __shared__ SceneLds lds;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t o = P.off[b];
    const int n = P.counters[b * 2], f = P.counters[b * 2 + 1];
    const int np = P.npoints;
    if (tid == 0) P.nvalid[b] = n;
    if (n == 0) {
        scene_empty_frame(P, b, P.out_int, nullptr);
        return;
    }
    const SceneSel ss = scene_select_sort(P.list + o, n, f, np, P.NP, P.seed, (unsigned)b, keys, lds);
    // ---- rows in shuffled order (a short selection -- status 1 -- repeats cyclically)
    for (int j = tid; j < np; j += SCENE_THREADS) scene_write_row(P, b, o, j, (unsigned)keys[lds_phys(j < ss.total ? j : j % ss.total)]);
    if (tid == 0) P.status[b] = ss.status;
}

// ---- 16384 < npoints <= 65536 ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCENE_THREADS) void scene_select_large_kernel(SceneParams P) {
    __shared__ SceneLds lds;
    const int b = blockIdx.x;
    scene_select_large(P, b, P.list + P.off[b], P.out_int, nullptr, lds);
}

// The bitonic network of proposal.hip's large score sort on every frame's NP keys: SCENE_SMALL_MAX-key chunks sorted in LDS (chunk c
// descending when c is odd: the bitonic building blocks), then per stage k the strides >= SCENE_SMALL_MAX as compare-exchange passes
// in HBM and the rest as one LDS merge per chunk.  A descending sort / merge is an ascending one on the complemented keys.
// Frames whose total is 0 are skipped.  grid (NP / SCENE_SMALL_MAX, B) x 1024 threads, 16 keys each.
__global__ __launch_bounds__(SCENE_THREADS) void scene_chunk_sort_kernel(u64* __restrict__ all_keys, const int32_t* __restrict__ total, int NP) {
    extern __shared__ u64 keys[];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    if (total[b] == 0) return;
    const bool desc = c & 1;
    u64* o = all_keys + (size_t)b * NP + (size_t)c * SCENE_SMALL_MAX + t * 16;
    u64 v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = desc ? ~o[e] : o[e];
    block_sort16(v, keys, SCENE_SMALL_MAX, t);
#pragma unroll
    for (int e = 0; e < 16; e++) o[e] = desc ? ~v[e] : v[e];
}
// grid (NP / 2 / 256, B) x 256 threads, one pair each
__global__ __launch_bounds__(256) void scene_cx_kernel(u64* __restrict__ all_keys, const int32_t* __restrict__ total, int NP, int j, int k) {
    const int b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= (NP >> 1) || total[b] == 0) return;
    u64* w = all_keys + (size_t)b * NP;
    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    const u64 a = w[i], c = w[i + j];
    const bool up = (i & k) == 0;
    if ((a > c) == up) { w[i] = c; w[i + j] = a; }
}
__global__ __launch_bounds__(SCENE_THREADS) void scene_chunk_merge_kernel(u64* __restrict__ all_keys, const int32_t* __restrict__ total, int NP, int k) {
    extern __shared__ u64 keys[];
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    if (total[b] == 0) return;
    const bool desc = ((c * SCENE_SMALL_MAX) & k) != 0;
    u64* o = all_keys + (size_t)b * NP + (size_t)c * SCENE_SMALL_MAX + t * 16;
    u64 v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = desc ? ~o[e] : o[e];
    block_merge16(v, keys, SCENE_SMALL_MAX, t);
#pragma unroll
    for (int e = 0; e < 16; e++) o[e] = desc ? ~v[e] : v[e];
}

int scene_large_shuffle(const char* who, const SceneFrames& F, hipStream_t s) {
    static PrcnnLdsLimit attr_sort, attr_merge;
    const int lds = (int)lds_sort_bytes(SCENE_SMALL_MAX);
    if (!attr_sort.raise((const void*)scene_chunk_sort_kernel, lds) || !attr_merge.raise((const void*)scene_chunk_merge_kernel, lds))
        return prcnn_fail(PRCNN_EHIP, "%s: cannot raise the dynamic LDS limit", who);
    const int NP = F.NP, B = F.B;
    const dim3 chunks(NP / SCENE_SMALL_MAX, B), pairs(NP / 2 / 256, B);
    hipLaunchKernelGGL(scene_chunk_sort_kernel, chunks, dim3(SCENE_THREADS), lds, s, F.large_keys, F.large_total, NP);
    for (int k = 2 * SCENE_SMALL_MAX; k <= NP; k <<= 1) {
        for (int j = k >> 1; j >= SCENE_SMALL_MAX; j >>= 1)
            hipLaunchKernelGGL(scene_cx_kernel, pairs, dim3(256), 0, s, F.large_keys, F.large_total, NP, j, k);
        hipLaunchKernelGGL(scene_chunk_merge_kernel, chunks, dim3(SCENE_THREADS), lds, s, F.large_keys, F.large_total, NP, k);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return prcnn_fail(PRCNN_EHIP, "%s(shuffle): launch failed: %s", who, hipGetErrorString(e));
    return PRCNN_OK;
}

// grid (ceil(npoints / SCENE_THREADS), B): one thread per output row
__global__ __launch_bounds__(SCENE_THREADS) void scene_rows_kernel(SceneParams P) {
    const int b = blockIdx.y, j = blockIdx.x * SCENE_THREADS + threadIdx.x;
    const int total = P.large_total[b];
    if (j >= P.npoints || total == 0) return;
    scene_write_row(P, b, P.off[b], j, scene_large_identity(P, b, j, total));
}

PRCNN_API size_t prcnn_scene_workspace_bytes(int64_t total_points, int B) {
    if (total_points < 0 || B < 0) return 0;
    return (size_t)total_points * sizeof(uint2) + scene_counters_bytes(B) + 64;      // 64: the list starts on a 64-byte boundary
}

// both exports; max_npoints = the export's domain
static int scene_prepare_any(const char* who, int max_npoints, const float* raw, const int64_t* offsets, int B, int64_t total_points,
                             int max_points_per_frame, const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                             float* out_xyz, float* out_intensity, int32_t* out_src, int32_t* nvalid, int32_t* status, void* workspace,
                             size_t workspace_bytes, prcnn_stream_t stream) {
    if (max_npoints == SCENE_SMALL_MAX)
        PRCNN_REQUIRE(npoints > 0 && npoints <= 16384, "%s: npoints=%d (1..16384: the shuffle is one LDS-resident sort per frame)", who, npoints);
    else
        PRCNN_REQUIRE(npoints > 0 && npoints <= SCENE_LARGE_MAX, "%s: npoints=%d (1..65536: the shuffle sorts at most four 16384-key chunks per frame)", who, npoints);
    const bool large = npoints > SCENE_SMALL_MAX;
    int rc = scene_check_frames(who, raw, offsets, B, total_points, max_points_per_frame, calib, 0, SCENE_THREADS);
    if (rc != PRCNN_OK || B == 0) return rc;
    PRCNN_REQUIRE(img_hw && out_xyz && out_intensity && out_src && nvalid && status, "%s: null pointer", who);
    const size_t small_bytes = prcnn_scene_workspace_bytes(total_points, B);
    PRCNN_REQUIRE(workspace && workspace_bytes >= scene_large_bytes(small_bytes, B, npoints), "%s: workspace too small", who);
    PRCNN_REQUIRE(!large || ((uintptr_t)workspace % 8) == 0, "%s: workspace must be 8-byte aligned", who);
    hipStream_t s = (hipStream_t)stream;
    SceneParams P = {};
    scene_fill_frames(P, raw, offsets, B, calib, img_hw, scope, npoints, seed, workspace, out_xyz, out_src, nvalid, status);
    if (large) scene_fill_large(P, workspace, small_bytes);
    P.out_int = out_intensity;
    if ((rc = scene_reset_counters(who, P, s)) != PRCNN_OK) return rc;
    if (max_points_per_frame > 0) {
        hipLaunchKernelGGL(scene_flag_kernel, dim3(prcnn_divup(max_points_per_frame, SCENE_THREADS), B), dim3(SCENE_THREADS), 0, s, P);
        PRCNN_LAUNCH_CHECK("prcnn_scene_prepare(flags)");
    }
    if (!large) return scene_launch_sample<scene_sample_kernel>(who, P, s);
    hipLaunchKernelGGL(scene_select_large_kernel, dim3(B), dim3(SCENE_THREADS), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_scene_prepare_large(select)");
    if ((rc = scene_large_shuffle(who, P, s)) != PRCNN_OK) return rc;
    hipLaunchKernelGGL(scene_rows_kernel, dim3(prcnn_divup(npoints, SCENE_THREADS), B), dim3(SCENE_THREADS), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_scene_prepare_large(rows)");
    return PRCNN_OK;
}

PRCNN_API int prcnn_scene_prepare(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                  const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                                  float* out_xyz, float* out_intensity, int32_t* out_src, int32_t* nvalid, int32_t* status,
                                  void* workspace, size_t workspace_bytes, prcnn_stream_t stream) {
    return scene_prepare_any("prcnn_scene_prepare", SCENE_SMALL_MAX, raw, offsets, B, total_points, max_points_per_frame, calib, img_hw, scope, npoints,
                             seed, out_xyz, out_intensity, out_src, nvalid, status, workspace, workspace_bytes, stream);
}

PRCNN_API size_t prcnn_scene_large_workspace_bytes(int64_t total_points, int B, int npoints) {
    if (total_points < 0 || B < 0 || npoints < 0) return 0;
    return scene_large_bytes(prcnn_scene_workspace_bytes(total_points, B), B, npoints);
}

PRCNN_API int prcnn_scene_prepare_large(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                        const float* calib, const int32_t* img_hw, const double* scope, int npoints, uint32_t seed,
                                        float* out_xyz, float* out_intensity, int32_t* out_src, int32_t* nvalid, int32_t* status,
                                        void* workspace, size_t workspace_bytes, prcnn_stream_t stream) {
    return scene_prepare_any("prcnn_scene_prepare_large", SCENE_LARGE_MAX, raw, offsets, B, total_points, max_points_per_frame, calib, img_hw, scope,
                             npoints, seed, out_xyz, out_intensity, out_src, nvalid, status, workspace, workspace_bytes, stream);
}
