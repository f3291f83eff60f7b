// grid.hip -- neighbour search over a per-frame uniform grid: ball_query / three_nn with the SAME results as the
// brute-force scans of neighbor.hip (and of the reference's CUDA ops), but touching only the cells a query can reach.
//
// The reference (and neighbor.hip) test every query against every point of the frame: 67 M distance evaluations per
// frame for SA1's ball query and again for FP0's three_nn, so the only way further at those sizes is to
// not do the work.  Points are binned once per frame into a 64x64
// (three_nn) or 128x128 (ball query) grid over the x-z plane (the LiDAR ground plane; y spans a few metres) and stored cell-contiguous as float4
// (x, y, z, original index); a query then visits the 3x3-ish block of cells its ball overlaps (ball_query) or grows a
// square ring by ring until the third-best distance is provably final (three_nn): ~30 candidates instead of 16 384.
//
// Exactness: every candidate is tested with the canonical distance arithmetic of neighbor.hip (common.h sqdist3), the
// candidate cell range is a superset of the ball by monotonicity of the cell function, and both result rules are
// restated order-independently --
//   ball_query: "first nsample hits in index order, padded with the first hit" == the nsample SMALLEST indices among
//               the hits, ascending, padded with the smallest;
//   three_nn  : strict-'<' insertion in index order == the three smallest (d2, index) pairs, lexicographically
// -- so the output is bit-identical to the scan regardless of the (arbitrary) order of points inside a cell.
//
// Where the time went and what each kernel does about it:
//   grid_build_kernel      one workgroup per frame; a thread reads its points ONCE, all loads in flight together, and keeps
//                          them in registers through the bounds, count and scatter passes (three dependent sweeps before);
//                          its chain of barriers and LDS passes is the time: one reduction for the four bounds, counters and
//                          cell starts moved as int4
//   grid_ball_query_kernel a workgroup whose frame is flagged dense runs the index-order scan itself (grid_layout.h): one
//                          launch, where a second scan launch used to retire B * M / 64 workgroups that exit at once
//   grid_three_nn_kernel   a 64x64 grid of up to 4 096 points (80 KB) is staged into LDS once per workgroup; the dependent
//                          chain cell_start[c] -> cell_start[c + 1] -> points of every visited cell then runs at LDS
//                          latency, not through L2 with 64 unrelated cells per wave; the two runs of cells of a ring step
//                          share one look-up and one loop
#include "grid_layout.h"

#define GRID_BUILD_THREADS 1024
#define GRID_BUILD_REG_PTS 16                    // points a thread holds in registers: frames of up to 16 384 points

__device__ __forceinline__ const int32_t* grid_cells(const void* g, size_t fb, int b) { return (const int32_t*)((const char*)g + fb * b + sizeof(GridHeader)); }
__device__ __forceinline__ const float4* grid_points(const void* g, size_t fb, int b) {
    size_t off = (sizeof(GridHeader) + (size_t)(GRID_CELLS_MAX + 1) * 4 + 15) & ~(size_t)15;
    return (const float4*)((const char*)g + fb * b + off);
}

// monotone non-decreasing in v for fixed (o, inv): fp32 subtract, multiply by a positive constant, truncate, clamp
__device__ __forceinline__ int cell_coord(float v, float o, float inv, int dim) {
    float t = (v - o) * inv;
    t = fminf(fmaxf(t, 0.0f), (float)(dim - 1));            // NaN -> 0
    return (int)t;
}

// the four bounds of the frame in one pass (one barrier pair, not four): wave butterflies, then the waves' values in wave order;
// scratch holds 4 floats per wave
__device__ __forceinline__ void block_reduce_bounds(float& mnx, float& mxx, float& mnz, float& mxz, float* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        mnx = fminf(mnx, __shfl_xor(mnx, d, 64)); mxx = fmaxf(mxx, __shfl_xor(mxx, d, 64));
        mnz = fminf(mnz, __shfl_xor(mnz, d, 64)); mxz = fmaxf(mxz, __shfl_xor(mxz, d, 64));
    }
    __syncthreads();
    if (lane == 0) { scratch[wave * 4] = mnx; scratch[wave * 4 + 1] = mxx; scratch[wave * 4 + 2] = mnz; scratch[wave * 4 + 3] = mxz; }
    __syncthreads();
    mnx = scratch[0]; mxx = scratch[1]; mnz = scratch[2]; mxz = scratch[3];
    for (int w = 1; w < nw; w++) {
        mnx = fminf(mnx, scratch[w * 4]); mxx = fmaxf(mxx, scratch[w * 4 + 1]);
        mnz = fminf(mnz, scratch[w * 4 + 2]); mxz = fmaxf(mxz, scratch[w * 4 + 3]);
    }
}

__device__ __forceinline__ float block_reduce_sum(float v, float* scratch) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < nw; w++) r += scratch[w];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(GRID_BUILD_THREADS) void grid_build_kernel(const float* __restrict__ xyz, int N, float min_cell, int dim,
                                                                        void* grid, size_t fb) {
    extern __shared__ __attribute__((aligned(16))) int cnt[];                  // dim * dim counters / scatter cursors
    const int ncell = dim * dim, per_thread4 = ncell / GRID_BUILD_THREADS / 4;       // 4 or 16 cells per thread, as int4: 1 or 4
    __shared__ float red[4 * GRID_BUILD_THREADS / 64];
    __shared__ int wsum[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ p = xyz + (size_t)b * N * 3;
    GridHeader* H = (GridHeader*)grid_header(grid, fb, b);
    int32_t* cstart = (int32_t*)grid_cells(grid, fb, b);
    float4* sorted = (float4*)grid_points(grid, fb, b);
    // The three passes over the frame (bounds, count, scatter) visit point tid + u * 1024 in the same order.  A frame of up
    // to 16 384 points is read once, every load issued before the first is needed, and stays in registers; a larger one is
    // read from memory in each pass.
    const bool inreg = N <= GRID_BUILD_REG_PTS * GRID_BUILD_THREADS;
    float px[GRID_BUILD_REG_PTS], py[GRID_BUILD_REG_PTS], pz[GRID_BUILD_REG_PTS];
    if (inreg) {
#pragma unroll
        for (int u = 0; u < GRID_BUILD_REG_PTS; u++) {
            const int i = tid + u * GRID_BUILD_THREADS;
            if (i < N) {
                const Trip<float> v = *reinterpret_cast<const Trip<float>*>(p + (size_t)i * 3);
                px[u] = v.a; py[u] = v.b; pz[u] = v.c;
            }
        }
    }
    auto for_points = [&](auto&& f) __attribute__((always_inline)) {
        if (inreg) {
#pragma unroll
            for (int u = 0; u < GRID_BUILD_REG_PTS; u++) {
                const int i = tid + u * GRID_BUILD_THREADS;
                if (i < N) f(i, px[u], py[u], pz[u]);
            }
        } else {
            for (int i = tid; i < N; i += GRID_BUILD_THREADS) f(i, p[i * 3], p[i * 3 + 1], p[i * 3 + 2]);
        }
    };
    // bounds over the finite points
    float mnx = INFINITY, mxx = -INFINITY, mnz = INFINITY, mxz = -INFINITY;
    for_points([&](int, float x, float, float z) {
        if (fabsf(x) < INFINITY && fabsf(z) < INFINITY) {
            mnx = fminf(mnx, x); mxx = fmaxf(mxx, x); mnz = fminf(mnz, z); mxz = fmaxf(mxz, z);
        }
    });
    block_reduce_bounds(mnx, mxx, mnz, mxz, red);
    if (!(mnx <= mxx)) { mnx = mxx = 0.f; mnz = mxz = 0.f; }           // no finite point at all
    float cs = fmaxf(fmaxf(mxx - mnx, mxz - mnz) / (float)dim * 1.0001f, fmaxf(min_cell, 1e-3f));
    const float inv = 1.0f / cs;
    for (int c = tid; c < ncell / 4; c += GRID_BUILD_THREADS) reinterpret_cast<int4*>(cnt)[c] = make_int4(0, 0, 0, 0);
    __syncthreads();
    for_points([&](int, float x, float, float z) {
        int c = cell_coord(z, mnz, inv, dim) * dim + cell_coord(x, mnx, inv, dim);
        atomicAdd(&cnt[c], 1);
    });
    __syncthreads();
    // exclusive scan of the counts: per_thread consecutive cells per thread, wave scan, wave offsets
    // (the thread's counters and cell starts move as int4: a quarter of the LDS and store instructions, and whole 16-byte
    //  pieces of a line per store where single ints went out at a 16- or 64-byte stride)
    int4* cnt4 = reinterpret_cast<int4*>(cnt) + tid * per_thread4;
    int4* cstart4 = reinterpret_cast<int4*>(cstart) + tid * per_thread4;       // frame blocks and the header: multiples of 16 bytes
    int ssum = 0, occ = 0;
    for (int u = 0; u < per_thread4; u++) {
        const int4 c = cnt4[u];
        ssum += (c.x + c.y) + (c.z + c.w);
        occ += (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0);
    }
    const float occupied = block_reduce_sum((float)occ, red);
    int inc = ssum;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int woff = 0;
    for (int w = 0; w < wave; w++) woff += wsum[w];
    int run = woff + inc - ssum;
    for (int u = 0; u < per_thread4; u++) {
        const int4 c = cnt4[u];
        const int4 st = make_int4(run, run + c.x, run + c.x + c.y, run + c.x + c.y + c.z);
        cstart4[u] = st;
        cnt4[u] = st;                            // becomes the scatter cursor
        run = st.w + c.w;
    }
    if (tid == GRID_BUILD_THREADS - 1) cstart[ncell] = run;
    if (tid == 0) {
        H->x0 = mnx; H->z0 = mnz; H->inv_cs = inv; H->cs = cs; H->dim = dim;
        const float side = 2.0f * min_cell * inv + 1.0f;                       // cells a ball of radius min_cell spans per axis
        H->cand = (float)N / fmaxf(occupied, 1.0f) * side * side;
        H->pad1 = H->pad2 = 0;
    }
    __syncthreads();
    for_points([&](int i, float x, float y, float z) {
        int c = cell_coord(z, mnz, inv, dim) * dim + cell_coord(x, mnx, inv, dim);
        int pos = atomicAdd(&cnt[c], 1);
        sorted[pos] = make_float4(x, y, z, __int_as_float(i));
    });
}

// ---- ball query over the grid: one thread per centroid, per-thread sorted hit lists in LDS (k-major) ----------
#define GBQ_THREADS 64
static_assert(GBQ_THREADS == BQ_THREADS, "a dense frame's workgroups run the scan of neighbor.hip: same block, same grid");

// keep the `cap` smallest indices, ascending; returns the new count
__device__ __forceinline__ int insert_sorted(int* list, int stride, int cnt, int cap, int k) {
    if (cnt == cap) {
        if (k >= list[(cap - 1) * stride]) return cnt;
        cnt = cap - 1;                            // the largest falls off
    }
    int pos = cnt;
    while (pos > 0 && list[(pos - 1) * stride] > k) { list[pos * stride] = list[(pos - 1) * stride]; pos--; }
    list[pos * stride] = k;
    return cnt + 1;
}

// xyz != nullptr: a workgroup of a frame the build flagged dense answers its 64 centroids with the index-order scan (same
// results); the hit lists are not used then and the scan stages its chunks in their place (the host sizes the dynamic LDS
// for the larger of the two).
template <bool DUAL>
__global__ __launch_bounds__(GBQ_THREADS) void grid_ball_query_kernel(const void* __restrict__ grid, size_t fb,
                                                                     const float* __restrict__ xyz,
                                                                     const float* __restrict__ new_xyz, int M, float ra,
                                                                     float r2a, int nsa, int32_t* __restrict__ idxa, float rb,
                                                                     float r2b, int nsb, int32_t* __restrict__ idxb, int N) {
    extern __shared__ __attribute__((aligned(16))) int lists[];               // [nsa + nsb][GBQ_THREADS] | scan chunk
    const int b = blockIdx.y, tid = threadIdx.x;
    const GridHeader H = *grid_header(grid, fb, b);
    if (xyz && grid_frame_dense(H, N)) {          // uniform over the workgroup
        ball_query_scan_block<DUAL>(reinterpret_cast<float*>(lists), xyz, new_xyz, N, M, b, blockIdx.x, r2a, nsa, idxa, r2b, nsb, idxb);
        return;
    }
    const int m = blockIdx.x * GBQ_THREADS + tid;
    if (m >= M) return;
    const int32_t* __restrict__ cstart = grid_cells(grid, fb, b);
    const float4* __restrict__ pts = grid_points(grid, fb, b);
    const float* q = new_xyz + ((size_t)b * M + m) * 3;
    const float qx = q[0], qy = q[1], qz = q[2];
    int* la = lists + tid;
    int* lb = lists + nsa * GBQ_THREADS + tid;
    int cnta = 0, cntb = 0;
    const float rmax = DUAL ? fmaxf(ra, rb) : ra;
    const float r2max = DUAL ? fmaxf(r2a, r2b) : r2a;
    // a hit has |dx| < r (its squared distance, a sum of rounded non-negative terms, is below r2): widen r by a
    // relative margin that dwarfs the rounding of r*r and of the subtraction; cell_coord is monotone
    const float rs = rmax * 1.001f + 1e-6f;
    if (qx == qx && qz == qz && r2max > 0.0f) {   // NaN centroid: no hits
        const int dim = H.dim;
        const int cx0 = cell_coord(qx - rs, H.x0, H.inv_cs, dim), cx1 = cell_coord(qx + rs, H.x0, H.inv_cs, dim);
        const int cz0 = cell_coord(qz - rs, H.z0, H.inv_cs, dim), cz1 = cell_coord(qz + rs, H.z0, H.inv_cs, dim);
        for (int cz = cz0; cz <= cz1; cz++) {
            const int beg = cstart[cz * dim + cx0], end = cstart[cz * dim + cx1 + 1];   // one contiguous run per row
            for (int t = beg; t < end; t++) {
                const float4 c = pts[t];
                const float d = sqdist3(qx, qy, qz, c.x, c.y, c.z);
                if (d < r2max) {
                    const int k = __float_as_int(c.w);
                    if (d < r2a) cnta = insert_sorted(la, GBQ_THREADS, cnta, nsa, k);
                    if (DUAL && d < r2b) cntb = insert_sorted(lb, GBQ_THREADS, cntb, nsb, k);
                }
            }
        }
    }
    int32_t* oa = idxa + ((size_t)b * M + m) * nsa;
    const int fa = cnta ? la[0] : 0;
    for (int s = 0; s < nsa; s++) oa[s] = s < cnta ? la[s * GBQ_THREADS] : fa;
    if (DUAL) {
        int32_t* ob = idxb + ((size_t)b * M + m) * nsb;
        const int fbk = cntb ? lb[0] : 0;
        for (int s = 0; s < nsb; s++) ob[s] = s < cntb ? lb[s * GBQ_THREADS] : fbk;
    }
}

// ---- three_nn over the grid: one thread per query, square rings until the third-best distance is final -------
#define GNN_THREADS 256                           // block of the global-memory path
#define GNN_LDS_THREADS 1024                      // largest block of the staged path (the host halves it on small launches)
#define GNN_LDS_DIM 64                            // the grid that is staged: 64 x 64 cells ...
#define GNN_LDS_MAX_M 4096                        // ... of at most 4 096 points: 64 KB of float4 + 16.4 KB of cell starts
#define GNN_LDS_CELL_BYTES (((GNN_LDS_DIM * GNN_LDS_DIM + 1) * 4 + 15) & ~15)

// The three nearest of (ux, uy, uz) among the frame's points.  `cstart` and `pts` are the frame's cell starts and sorted
// points, in global memory or staged in LDS: the function is inlined at both call sites, so each gets the loads of its own
// address space; the ring logic and the arithmetic are the same.
__device__ __forceinline__ void grid_three_nn_rings(const GridHeader& H, const int32_t* __restrict__ cstart, const float4* __restrict__ pts,
                                                    float ux, float uy, float uz, float& b1, float& b2, float& b3, int& i1, int& i2,
                                                    int& i3) {
    const int GD = H.dim;
    // always_inline: as an out-of-line call the by-reference captures (the running top-3) live in scratch memory
    // Two runs of cells per call -- the ring's bottom and top rows, or the left and right cell of one of its other rows; oka / okb:
    // the run lies inside the grid.  The four cell starts are read together and the two runs of points share ONE loop: its trip
    // count in a wave is the largest SUM over the lanes, where two loops cost the sum of the two largest counts, and a ring
    // costs half the dependent look-ups.  The order in which candidates are seen does not matter (header).
    auto visit2 = [&](bool oka, int cza, int cxa0, int cxa1, bool okb, int czb, int cxb0, int cxb1) __attribute__((always_inline)) {
        const int bega = cstart[oka ? cza * GD + cxa0 : 0], enda = cstart[oka ? cza * GD + cxa1 + 1 : 0];
        const int begb = cstart[okb ? czb * GD + cxb0 : 0], endb = cstart[okb ? czb * GD + cxb1 + 1 : 0];
        const int na = enda - bega, nb = endb - begb;
        for (int j = 0; j < na + nb; j++) {
            const float4 c = pts[j < na ? bega + j : begb + (j - na)];
            const float dd = sqdist3(ux, uy, uz, c.x, c.y, c.z);
            const int k = __float_as_int(c.w);
            // lexicographic (distance, index): what strict-'<' insertion in index order produces
            // (written with selects: as an if / else-if ladder the compiler turned the six running values into a
            //  dynamically indexed array in scratch memory)
            if (dd < b3 || (dd == b3 && k < i3 && dd < INFINITY)) {
                const bool lt1 = dd < b1 || (dd == b1 && k < i1);
                const bool lt2 = lt1 || dd < b2 || (dd == b2 && k < i2);
                b3 = lt2 ? b2 : dd; i3 = lt2 ? i2 : k;
                b2 = lt1 ? b1 : (lt2 ? dd : b2); i2 = lt1 ? i1 : (lt2 ? k : i2);
                b1 = lt1 ? dd : b1; i1 = lt1 ? k : i1;
            }
        }
    };
    const bool finite_q = fabsf(ux) < INFINITY && fabsf(uz) < INFINITY;
    if (!finite_q) return;
    // unclamped cell coordinates of the query (it may lie outside the grid's bounding box)
    const float fx = (ux - H.x0) * H.inv_cs, fz = (uz - H.z0) * H.inv_cs;
    // A query outside the points' bounding box starts from the ring just outside the grid ([-1, GD]) on that side: the
    // bounds below measure from the query's real coordinates to cell sides, so they stay valid, and a far-away query
    // costs at most GD rings instead of one ring per cell of its distance.
    const int qcx = (int)floorf(fminf(fmaxf(fx, -1.0f), (float)GD)), qcz = (int)floorf(fminf(fmaxf(fz, -1.0f), (float)GD));
    for (int R = 0;; R++) {
        const int x0 = qcx - R, x1 = qcx + R, z0 = qcz - R, z1 = qcz + R;
        const int cxa = max(x0, 0), cxb = min(x1, GD - 1);
        visit2(cxa <= cxb && z0 >= 0 && z0 < GD, z0, cxa, cxb,                       // bottom row of the ring
               cxa <= cxb && R > 0 && z1 >= 0 && z1 < GD, z1, cxa, cxb);             // top row
        if (R > 0) {                                                                  // left / right columns
            const int za = max(z0 + 1, 0), zb = min(z1 - 1, GD - 1);
            const bool okl = x0 >= 0 && x0 < GD, okr = x1 >= 0 && x1 < GD;
            if (okl || okr)
                for (int cz = za; cz <= zb; cz++) visit2(okl, cz, x0, x0, okr, cz, x1, x1);
        }
        if (x0 <= 0 && z0 <= 0 && x1 >= GD - 1 && z1 >= GD - 1) break;    // whole grid visited
        // every point not yet visited lies outside the square of cells [x0,x1] x [z0,z1]; points are binned by a
        // CLAMPED coordinate, so only sides strictly inside the grid bound anything.  Planar distance from the
        // query to the nearest such side, shrunk by a margin far above the rounding of the cell arithmetic:
        float lb = INFINITY;
        if (x0 > 0) lb = fminf(lb, ux - (H.x0 + (float)x0 * H.cs));
        if (x1 < GD - 1) lb = fminf(lb, (H.x0 + (float)(x1 + 1) * H.cs) - ux);
        if (z0 > 0) lb = fminf(lb, uz - (H.z0 + (float)z0 * H.cs));
        if (z1 < GD - 1) lb = fminf(lb, (H.z0 + (float)(z1 + 1) * H.cs) - uz);
        lb = lb * 0.999f - 1e-4f * H.cs;
        if (lb > 0.0f && b3 < lb * lb) break;
    }
}

// A workgroup answers queries [blockIdx.x * qpb, +qpb) of frame blockIdx.y, blockDim.x at a time.  lds_m != 0 (the frame's
// point count, <= GNN_LDS_MAX_M): the dynamic LDS holds lds_m float4 and GNN_LDS_CELL_BYTES of cell starts, and a frame whose
// grid has GNN_LDS_DIM cells per axis is staged there once and searched from there; any other grid is searched in place.
__global__ __launch_bounds__(GNN_LDS_THREADS) void grid_three_nn_kernel(const void* __restrict__ grid, size_t fb,
                                                                        const float* __restrict__ unknown, int n, int qpb, int lds_m,
                                                                        float* __restrict__ dist2, int32_t* __restrict__ idx,
                                                                        float* __restrict__ weight) {
    extern __shared__ __attribute__((aligned(16))) char gsm[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const GridHeader H = *grid_header(grid, fb, b);
    const int32_t* __restrict__ cstart = grid_cells(grid, fb, b);
    const float4* __restrict__ pts = grid_points(grid, fb, b);
    float4* spts = reinterpret_cast<float4*>(gsm);
    int32_t* scell = reinterpret_cast<int32_t*>(gsm + (size_t)lds_m * sizeof(float4));
    const bool staged = lds_m != 0 && H.dim == GNN_LDS_DIM;              // uniform over the workgroup
    if (staged) {
        for (int t = tid; t < lds_m; t += blockDim.x) spts[t] = pts[t];
        const int4* csrc = reinterpret_cast<const int4*>(cstart);        // frame blocks and the header are multiples of 16 bytes
        int4* cdst = reinterpret_cast<int4*>(scell);
        for (int t = tid; t < GNN_LDS_DIM * GNN_LDS_DIM / 4; t += blockDim.x) cdst[t] = csrc[t];
        if (tid == 0) scell[GNN_LDS_DIM * GNN_LDS_DIM] = cstart[GNN_LDS_DIM * GNN_LDS_DIM];
        __syncthreads();
    }
    const int qend = min(n, (blockIdx.x + 1) * qpb);
    for (int i = blockIdx.x * qpb + tid; i < qend; i += blockDim.x) {
        const float* u = unknown + ((size_t)b * n + i) * 3;
        const float ux = u[0], uy = u[1], uz = u[2];
        float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
        int i1 = 0, i2 = 0, i3 = 0;
        if (staged) grid_three_nn_rings(H, scell, spts, ux, uy, uz, b1, b2, b3, i1, i2, i3);
        else grid_three_nn_rings(H, cstart, pts, ux, uy, uz, b1, b2, b3, i1, i2, i3);
        // a query's three values are 12 contiguous bytes of each output: ONE global_store_dwordx3 per array (a wave then writes
        // 768 contiguous bytes per instruction; nine 4-byte stores at a 12-byte stride measured 10x write amplification)
        const size_t o = ((size_t)b * n + i) * 3;
        *reinterpret_cast<Trip<float>*>(dist2 + o) = Trip<float>{b1, b2, b3};
        *reinterpret_cast<Trip<int32_t>*>(idx + o) = Trip<int32_t>{i1, i2, i3};
        if (weight) {                                 // same expressions as three_nn_kernel (neighbor.hip)
            float r0 = 1.0f / (sqrtf(b1) + 1e-8f);
            float r1 = 1.0f / (sqrtf(b2) + 1e-8f);
            float r2 = 1.0f / (sqrtf(b3) + 1e-8f);
            float s = (r0 + r1) + r2;
            *reinterpret_cast<Trip<float>*>(weight + o) = Trip<float>{r0 / s, r1 / s, r2 / s};
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------
PRCNN_API size_t prcnn_grid_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return grid_frame_bytes(N) * (size_t)B;
}

PRCNN_API int prcnn_grid_build(const float* xyz, int B, int N, float min_cell, int cells_per_axis, void* grid, size_t grid_bytes,
                               prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && N > 0 && min_cell >= 0.0f, "prcnn_grid_build: bad shape B=%d N=%d min_cell=%g", B, N, (double)min_cell);
    PRCNN_REQUIRE(cells_per_axis == 64 || cells_per_axis == 128, "prcnn_grid_build: cells_per_axis must be 64 or 128, got %d", cells_per_axis);
    if (B == 0) return PRCNN_OK;
    PRCNN_REQUIRE(xyz && grid, "prcnn_grid_build: null pointer");
    PRCNN_REQUIRE(((uintptr_t)grid & 15) == 0, "prcnn_grid_build: grid buffer must be 16-byte aligned");
    PRCNN_REQUIRE(grid_bytes >= prcnn_grid_bytes(B, N), "prcnn_grid_build: buffer %zu < %zu bytes", grid_bytes, prcnn_grid_bytes(B, N));
    static PrcnnLdsLimit attr;
    if (!attr.raise((const void*)grid_build_kernel, GRID_CELLS_MAX * 4))
        return prcnn_fail(PRCNN_EHIP, "prcnn_grid_build: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL(grid_build_kernel, dim3(B), dim3(GRID_BUILD_THREADS), (size_t)cells_per_axis * cells_per_axis * 4, (hipStream_t)stream,
                       xyz, N, min_cell, cells_per_axis, grid, grid_frame_bytes(N));
    PRCNN_LAUNCH_CHECK("prcnn_grid_build");
    return PRCNN_OK;
}

PRCNN_API int prcnn_ball_query2_grid(const void* grid, const float* xyz, const float* new_xyz, int B, int N, int M, float radius_a,
                                     int nsample_a, int32_t* idx_a, float radius_b, int nsample_b, int32_t* idx_b, prcnn_stream_t stream) {
    const bool dual = nsample_b > 0;
    PRCNN_REQUIRE(B >= 0 && N > 0 && M >= 0 && nsample_a > 0 && nsample_b >= 0, "prcnn_ball_query2_grid: bad shape");
    if (B == 0 || M == 0) return PRCNN_OK;
    PRCNN_REQUIRE(grid && new_xyz && idx_a && (!dual || idx_b), "prcnn_ball_query2_grid: null pointer");
    size_t lds = (size_t)(nsample_a + nsample_b) * GBQ_THREADS * sizeof(int);
    PRCNN_REQUIRE(lds <= 64 * 1024, "prcnn_ball_query2_grid: nsample %d+%d too large for the LDS hit lists", nsample_a, nsample_b);
    // dense frames (GridHeader::cand) are answered by the index-order scan inside the same launch; its chunk takes the lists' place
    if (xyz && lds < NB_CHUNK_BYTES) lds = NB_CHUNK_BYTES;
    dim3 g(prcnn_divup(M, GBQ_THREADS), B);
    const float r2a = radius_a * radius_a, r2b = radius_b * radius_b;      // fp32 products, as the oracle
    if (dual)
        hipLaunchKernelGGL(grid_ball_query_kernel<true>, g, dim3(GBQ_THREADS), lds, (hipStream_t)stream, grid, grid_frame_bytes(N),
                           xyz, new_xyz, M, radius_a, r2a, nsample_a, idx_a, radius_b, r2b, nsample_b, idx_b, N);
    else
        hipLaunchKernelGGL(grid_ball_query_kernel<false>, g, dim3(GBQ_THREADS), lds, (hipStream_t)stream, grid, grid_frame_bytes(N),
                           xyz, new_xyz, M, radius_a, r2a, nsample_a, idx_a, 0.f, 0.f, 0, (int32_t*)nullptr, N);
    PRCNN_LAUNCH_CHECK("prcnn_ball_query2_grid");
    return PRCNN_OK;
}

PRCNN_API int prcnn_three_nn_grid(const void* grid, const float* unknown, int B, int n, int m, float* dist2, int32_t* idx,
                                  float* weight, prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && n >= 0 && m > 0, "prcnn_three_nn_grid: bad shape B=%d n=%d m=%d", B, n, m);
    if (B == 0 || n == 0) return PRCNN_OK;
    PRCNN_REQUIRE(grid && unknown && dist2 && idx, "prcnn_three_nn_grid: null pointer");
    int threads = GNN_THREADS, qpb = GNN_THREADS, lds_m = 0;
    if (m <= GNN_LDS_MAX_M && ((uintptr_t)grid & 15) == 0) {
        // Staging costs every workgroup the frame's 16.4 KB + 16 m bytes: the largest block that still leaves the chip's 256
        // CUs a workgroup each, and two rounds of queries per block where even that leaves one per CU (FP0: 8 per frame).
        static PrcnnLdsLimit attr;
        if (!attr.raise((const void*)grid_three_nn_kernel, GNN_LDS_MAX_M * 16 + GNN_LDS_CELL_BYTES))
            return prcnn_fail(PRCNN_EHIP, "prcnn_three_nn_grid: cannot raise the dynamic LDS limit");
        threads = GNN_LDS_THREADS;
        while (threads > GNN_THREADS && (long)B * prcnn_divup(n, threads) < 256) threads >>= 1;
        qpb = threads;
        if (threads == GNN_LDS_THREADS && (long)B * prcnn_divup(n, 2 * threads) >= 256) qpb = 2 * threads;
        lds_m = m;
    }
    hipLaunchKernelGGL(grid_three_nn_kernel, dim3(prcnn_divup(n, qpb), B), dim3(threads), lds_m ? (size_t)lds_m * 16 + GNN_LDS_CELL_BYTES : 0,
                       (hipStream_t)stream, grid, grid_frame_bytes(m), unknown, n, qpb, lds_m, dist2, idx, weight);
    PRCNN_LAUNCH_CHECK("prcnn_three_nn_grid");
    return PRCNN_OK;
}
