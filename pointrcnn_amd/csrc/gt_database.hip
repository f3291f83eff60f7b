// gt_database.hip -- the GT-augmentation database built on the device: for a batch of frames, every labelled object's points.
//
// Replaces tools/generate_gt_database.py:50-84, which does per frame, in numpy and one extension call on one core: lidar_to_rect
// of the WHOLE scan (no FOV, image or PC_AREA_SCOPE filter), pts_in_boxes3d_cpu against the frame's kept label boxes, and per
// object a boolean-mask compaction of the rect points and intensities.  A point inside two boxes belongs to both objects.
//
// Arithmetic: nothing new.  rect = scene_rect of scene_common.h (the canonical lidar -> rect of scene.hip's contract); membership =
// make_box + pt_in_box<true> of box_test.h (roipool3d.cpp:82-95, with its 10 m gate), the test prcnn_pts_in_boxes3d runs.
//
// Order: an object's points appear in ascending raw index.  The output size depends on the data, so there are two passes over
// the scans and the caller allocates between them:
//   gtdb_kernel<false> (count): one 1024-thread block per (1024-point tile, frame).  The frame's BoxConsts sit in LDS; every thread
//                       transforms its point once and tests it against each box; the wave's ballot of box g goes to LDS, and the
//                       tile's hit count of (frame, box) -- the popcounts of its 16 ballots -- to the (frame, box, tile) table.
//                       npts (frame, box) is the integer sum of the tile counts (atomic adds of integers: any order, one result).
//   gtdb_scan_kernel  : one wave per (frame, box): exclusive prefix of the tile counts over the tiles.
//   gtdb_kernel<true> (fill): the same tiles recomputed; a hit's row = object offset (the caller's exclusive scan of npts) + tile
//                       prefix + prefix of the waves before its own + popcount of the ballot below its lane.  Positions come from
//                       prefixes only, never from the order of atomic appends: two runs write identical bytes.
// The fill pass checks every row against the size of the output buffers before it writes.
#include "scene_common.h"
#include "box_test.h"

constexpr int GTDB_THREADS = 1024;
constexpr int GTDB_WAVES = GTDB_THREADS / 64;
constexpr int GTDB_MAX_BOXES = 128;

struct GtdbParams {
    const float4* raw;          // (total, 4) x y z intensity, lidar frame
    const int64_t* off;         // (B+1) first raw point of every frame
    const float* calib;         // (B, 24): only M (4x3 row-major) is read
    const float* boxes;         // (B, G, 7)
    const int32_t* num_boxes;   // (B)
    int64_t total;
    int B, G, T;                // T tiles of GTDB_THREADS points cover max_points_per_frame
    int32_t* tile_cnt;          // (B, G, T) hits of (frame, box) in a tile
    int32_t* tile_off;          // (B, G, T) their exclusive prefix over the tiles
    int32_t* npts;              // (B, G)                       -- count pass
    const int64_t* obj_off;     // (B * G + 1)                  -- fill pass
    int64_t P;
    float* points;              // (P, 3)
    float* inten;               // (P)
    int32_t* src;               // (P)
};

// the frame's boxes and points as both passes see them; a frame whose offsets do not describe the raw buffer is empty
__device__ __forceinline__ int gtdb_frame(const GtdbParams& P, int b, int64_t& o, int& n) {
    o = P.off[b];
    int64_t n64 = P.off[b + 1] - o;
    if (o < 0 || n64 < 0 || o + n64 > P.total) n64 = 0;
    const int64_t cover = (int64_t)P.T * GTDB_THREADS;
    n = (int)(n64 < cover ? n64 : cover);
    return min(max(P.num_boxes[b], 0), P.G);
}

template <bool FILL>
__global__ __launch_bounds__(GTDB_THREADS) void gtdb_kernel(GtdbParams P) {
    __shared__ BoxConst sbox[GTDB_MAX_BOXES];
    __shared__ unsigned long long wmask[GTDB_WAVES][GTDB_MAX_BOXES];
    __shared__ int64_t sbase[GTDB_MAX_BOXES];
    __shared__ int wbase[GTDB_WAVES][GTDB_MAX_BOXES];
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t o;
    int n;
    const int nb = gtdb_frame(P, b, o, n);
    if (nb == 0) return;
    const size_t row0 = (size_t)b * P.G * P.T + t;                     // (b, g, t) sits at row0 + g * T
    if ((int64_t)t * GTDB_THREADS >= n) {
        if (!FILL && tid < nb) P.tile_cnt[row0 + (size_t)tid * P.T] = 0;
        return;
    }
    if (tid < nb) sbox[tid] = make_box(P.boxes + ((size_t)b * P.G + tid) * 7);
    __syncthreads();
    const int i = t * GTDB_THREADS + tid;
    const bool live = i < n;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        p = P.raw[o + i];
        scene_rect(p, P.calib + b * 24, x, y, z);
    }
    for (int g = 0; g < nb; g++) {
        const bool hit = live && pt_in_box<true>(sbox[g], x, y, z);
        const unsigned long long bv = __ballot(hit);
        if (lane == 0) wmask[wave][g] = bv;
    }
    __syncthreads();
    if (!FILL) {
        if (tid < nb) {
            int c = 0;
            for (int w = 0; w < GTDB_WAVES; w++) c += (int)__popcll(wmask[w][tid]);
            P.tile_cnt[row0 + (size_t)tid * P.T] = c;
            if (c > 0) atomicAdd(P.npts + b * P.G + tid, c);
        }
        return;
    }
    if (tid < nb) {
        int c = 0;
        for (int w = 0; w < GTDB_WAVES; w++) {
            wbase[w][tid] = c;
            c += (int)__popcll(wmask[w][tid]);
        }
        sbase[tid] = P.obj_off[(size_t)b * P.G + tid] + P.tile_off[row0 + (size_t)tid * P.T];
    }
    __syncthreads();
    for (int g = 0; g < nb; g++) {
        const unsigned long long bv = wmask[wave][g];
        if (bv == 0ULL) continue;
        if ((bv >> lane) & 1ULL) {
            const int64_t pos = sbase[g] + wbase[wave][g] + (int)__popcll(bv & ((1ULL << lane) - 1ULL));
            if (pos >= 0 && pos < P.P) {
                P.points[pos * 3 + 0] = x;
                P.points[pos * 3 + 1] = y;
                P.points[pos * 3 + 2] = z;
                P.inten[pos] = p.w;
                P.src[pos] = i;
            }
        }
    }
}

__global__ __launch_bounds__(64) void gtdb_scan_kernel(GtdbParams P) {
    const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
    if (g >= min(max(P.num_boxes[b], 0), P.G)) return;
    const size_t row = ((size_t)b * P.G + g) * P.T;
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
}

static size_t gtdb_table_bytes(int64_t max_points_per_frame, int B, int G) {
    const size_t T = (size_t)((max_points_per_frame + GTDB_THREADS - 1) / GTDB_THREADS);
    return (((size_t)B * G * T * sizeof(int32_t) + 63) / 64) * 64;
}

PRCNN_API size_t prcnn_gt_database_workspace_bytes(int64_t max_points_per_frame, int B, int G) {
    if (max_points_per_frame < 0 || B < 0 || G < 0) return 0;
    return 2 * gtdb_table_bytes(max_points_per_frame, B, G) + 64;
}

// what both entry points require of the arguments they share; fills P
static int gtdb_common(const char* who, GtdbParams& P, const float* raw, const int64_t* offsets, int B, int64_t total_points,
                       int max_points_per_frame, const float* calib, const float* boxes3d, const int32_t* num_boxes, int G, void* workspace,
                       size_t workspace_bytes) {
    PRCNN_REQUIRE(B <= 65535, "%s: bad shape B=%d total=%ld", who, B, (long)total_points);
    PRCNN_REQUIRE(G >= 0 && G <= GTDB_MAX_BOXES, "%s: G=%d (at most %d boxes per frame: their constants are LDS-resident)", who, G, GTDB_MAX_BOXES);
    const int rc = scene_check_frames(who, raw, offsets, B, total_points, max_points_per_frame, calib, 0, GTDB_THREADS, G == 0);
    if (rc != PRCNN_OK || B == 0 || G == 0) return rc;
    PRCNN_REQUIRE(boxes3d && num_boxes, "%s: null pointer", who);
    PRCNN_REQUIRE(workspace && ((uintptr_t)workspace % 4) == 0 && workspace_bytes >= prcnn_gt_database_workspace_bytes(max_points_per_frame, B, G),
                  "%s: workspace too small", who);
    P.raw = reinterpret_cast<const float4*>(raw); P.off = offsets; P.calib = calib; P.boxes = boxes3d; P.num_boxes = num_boxes;
    P.total = total_points; P.B = B; P.G = G; P.T = prcnn_divup(max_points_per_frame, GTDB_THREADS);
    char* w = static_cast<char*>(workspace);
    P.tile_cnt = reinterpret_cast<int32_t*>(w);
    P.tile_off = reinterpret_cast<int32_t*>(w + gtdb_table_bytes(max_points_per_frame, B, G));
    return PRCNN_OK;
}

PRCNN_API int prcnn_gt_database_count(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                      const float* calib, const float* boxes3d, const int32_t* num_boxes, int G, int32_t* npts,
                                      void* workspace, size_t workspace_bytes, prcnn_stream_t stream) {
    GtdbParams P = {};
    const int rc = gtdb_common("prcnn_gt_database_count", P, raw, offsets, B, total_points, max_points_per_frame, calib, boxes3d, num_boxes, G,
                               workspace, workspace_bytes);
    if (rc != PRCNN_OK || B == 0 || G == 0) return rc;
    PRCNN_REQUIRE(npts, "prcnn_gt_database_count: null pointer");
    hipStream_t s = (hipStream_t)stream;
    P.npts = npts;
    if (prcnn_fill_words(npts, 0u, (size_t)B * G, s) != hipSuccess) return prcnn_fail(PRCNN_EHIP, "prcnn_gt_database_count: memset failed");
    if (P.T == 0) return PRCNN_OK;
    hipLaunchKernelGGL(gtdb_kernel<false>, dim3(P.T, B), dim3(GTDB_THREADS), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_gt_database_count(count)");
    hipLaunchKernelGGL(gtdb_scan_kernel, dim3(G, B), dim3(64), 0, s, P);
    PRCNN_LAUNCH_CHECK("prcnn_gt_database_count(scan)");
    return PRCNN_OK;
}

PRCNN_API int prcnn_gt_database_fill(const float* raw, const int64_t* offsets, int B, int64_t total_points, int max_points_per_frame,
                                     const float* calib, const float* boxes3d, const int32_t* num_boxes, int G, const int64_t* obj_offsets,
                                     int64_t total_out, float* points, float* intensity, int32_t* src, void* workspace,
                                     size_t workspace_bytes, prcnn_stream_t stream) {
    GtdbParams P = {};
    const int rc = gtdb_common("prcnn_gt_database_fill", P, raw, offsets, B, total_points, max_points_per_frame, calib, boxes3d, num_boxes, G,
                               workspace, workspace_bytes);
    if (rc != PRCNN_OK || B == 0 || G == 0) return rc;
    PRCNN_REQUIRE(total_out >= 0, "prcnn_gt_database_fill: total_out=%ld", (long)total_out);
    if (total_out == 0 || P.T == 0) return PRCNN_OK;
    PRCNN_REQUIRE(obj_offsets && points && intensity && src, "prcnn_gt_database_fill: null pointer");
    P.obj_off = obj_offsets; P.P = total_out; P.points = points; P.inten = intensity; P.src = src;
    hipLaunchKernelGGL(gtdb_kernel<true>, dim3(P.T, B), dim3(GTDB_THREADS), 0, (hipStream_t)stream, P);
    PRCNN_LAUNCH_CHECK("prcnn_gt_database_fill");
    return PRCNN_OK;
}
