// mlp_multi.h -- the grouped stacks of one set-abstraction level in ONE launch (prcnn_mlp_chain_group_multi).
// Included once, at the bottom of mlp.hip after mlp_host.h (kernel bodies, decide_chain and the instance tables are above).
//
// The two radii of an MSG level are independent problems of the same structure, each with a flat row list and (SA1 / SA2) a
// dense list: three or four launches of 4-40 us that each leave most of the chip idle.  Here a workgroup looks up its problem
// in a table in the kernel arguments (level_units.h) and runs that problem's kernel body -- the SAME __device__ function the
// single launch runs, on the same rows: same bits.  The problems are decided one by one, as separate calls would be; a
// combination the tables below lack is PRCNN_EUNSUPPORTED.
#pragma once
#include "level_units.h"

struct MultiParams {
    LevelUnits U;
    int variant[LEVEL_MAX_PROBLEMS];        // which of the kernel's instantiated bodies problem p runs
    ChainParams c[LEVEL_MAX_PROBLEMS];
};
static_assert(sizeof(MultiParams) <= 4096, "the multi-problem kernels take their problems as kernel arguments");

// SA level 0: every row of SA0_TABLE is a body of the one kernel.  X(NB0 of one scale, NB0 of the other), wider first: the
// straight-line chains <group, NB0, 4, 0> (hoisted SA2 stacks) ...
#define FAST_MULTI_TABLE(X) X(3, 2)
// ... and X(NBW0, NBW0) of the two-layer stacks (SA3: 196 | 196 wide first layers; SA4: 384 | 256)
#define STACK_MULTI_TABLE(X) X(2, 2) X(3, 2)

enum {
#define X(W0, W1, NBL, NSV) SA0V_##W0##_##NSV,
    SA0_TABLE(X)
#undef X
    SA0V_COUNT
};

// (registers: those of the widest body, sa_xyz_chain_kernel<4, 4, 2, *>; the bodies use no LDS)
__global__ __launch_bounds__(256) void sa0_multi_kernel(const MultiParams M) {
    int prob, local, count;
    level_units_find(M.U, blockIdx.x, prob, local, count);
    switch (M.variant[prob]) {
#define X(W0, W1, NBL, NSV) case SA0V_##W0##_##NSV: sa_xyz_chain_body<W0 / 8, W1 / 8, NBL, NSV>(M.c[prob], local, count); break;
        SA0_TABLE(X)
#undef X
    }
}

// (one set of the chain's LDS arrays: their sizes do not depend on the instance)
template <int NBA, int NBB>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 8))) void chain_fast_multi_kernel(const MultiParams M) {
    FAST_CHAIN_LDS;
    int prob, local, count;
    level_units_find(M.U, blockIdx.x, prob, local, count);
    if (M.variant[prob] == 0) mlp_chain_fast_body<MODE_GROUP, NBA, 4, 0>(M.c[prob], local, Ws, s_wx, s_b, s_bias);
    else mlp_chain_fast_body<MODE_GROUP, NBB, 4, 0>(M.c[prob], local, Ws, s_wx, s_b, s_bias);
}

// (dynamic LDS: the larger of the problems' tiles; the layer-B split aims at ~256 live workgroups over the WHOLE launch)
// (waves per SIMD: the <2, 2> instance sits at the 256 registers of two and is held there; the wider one has never fitted them)
template <int NBWA, int NBWB>
__global__ __launch_bounds__(256, (NBWA <= 2 ? 2 : 1)) void stack2_multi_kernel(const MultiParams M) {
    extern __shared__ __attribute__((aligned(16))) float st_lds[];
    int prob, local, count;
    level_units_find(M.U, blockIdx.x, prob, local, count);
    int tiles_all = 0;
    for (int p = 0; p < M.U.nprob; p++) tiles_all += (int)((effective_rows(M.c[p].a) + ST_ROWS - 1) / ST_ROWS);
    if (NBWA == NBWB || M.variant[prob] == 0) mlp_stack2_body<NBWA>(M.c[prob], local, count, tiles_all, st_lds);
    else mlp_stack2_body<NBWB>(M.c[prob], local, count, tiles_all, st_lds);
}

#define STACK_MULTI_GRID_CAP 2048L          // the single launch's cap, for the whole launch

// dst / out2 / ld_out2 / col_off2: prcnn_mlp_chain_group_multi_dst's arguments (dst == NULL: every problem stores as it always has)
static int chain_group_multi(int nprob, const prcnn_chain_group_problem_t* prob, const int32_t* const* dst, float* out2, int ld_out2,
                             const int* col_off2, prcnn_stream_t stream) {
    PRCNN_REQUIRE(nprob >= 1 && nprob <= LEVEL_MAX_PROBLEMS && prob, "prcnn_mlp_chain_group_multi: nprob=%d (1..%d) or a null table", nprob,
                  LEVEL_MAX_PROBLEMS);
    PRCNN_REQUIRE(!dst || (out2 && col_off2 && ld_out2 > 0), "prcnn_mlp_chain_group_multi_dst: destination lists without an output to store to");
    MultiParams M = {};
    MlpLaunch L[LEVEL_MAX_PROBLEMS];
    int n = 0, family = K_NONE;
    for (int q = 0; q < nprob; q++) {
        const prcnn_chain_group_problem_t& a = prob[q];
        ChainParams& C = M.c[n];
        C = ChainParams{};
        int rc = fill_chain_group(C, a.xyz, a.new_xyz, a.idx, a.feat_cl, a.ld_feat, a.B, a.N, a.M, a.nsample, a.C, a.act_wx, a.act_bias, a.nlayers, a.wpack,
                                  a.bias, a.nout, a.relu, a.out, a.ld_out, a.col_off, a.pool_ns, a.groups_dev);
        if (rc) return rc;
        if (dst && dst[q]) {
            PRCNN_REQUIRE(col_off2[q] >= 0 && ld_out2 >= col_off2[q] + a.nout[a.nlayers - 1], "prcnn_mlp_chain_group_multi_dst: ld_out2=%d < col_off2+Nout of problem %d",
                          ld_out2, q);
            (a.pool_ns ? C.a.grp_dst : C.a.row_dst) = dst[q];
            C.a.out2 = out2; C.a.ld_out2 = ld_out2; C.a.col_off2 = col_off2[q];
        }
        L[n] = MlpLaunch();
        rc = decide_chain(MODE_GROUP, C, L[n]);
        if (rc) return rc;
        if (L[n].family == K_NONE) continue;                   // no rows
        const bool known = L[n].family == K_SA0 || L[n].family == K_CHAIN_FAST || L[n].family == K_STACK2;
        if (!known || L[n].block.x != 256 || (family != K_NONE && L[n].family != family)) return PRCNN_EUNSUPPORTED;
        family = L[n].family;
        n++;
    }
    if (n == 0) return PRCNN_OK;
    hipStream_t s = (hipStream_t)stream;
    long want[LEVEL_MAX_PROBLEMS] = {0, 0, 0, 0};
    for (int p = 0; p < n; p++) want[p] = L[p].grid.x;
    if (family == K_SA0) {
        for (int p = 0; p < n; p++) {
            M.variant[p] = -1;
#define X(W0, W1, NBL, NSV) if (L[p].a == W0 / 8 && L[p].b == W1 / 8 && L[p].c == NBL && L[p].d == NSV) M.variant[p] = SA0V_##W0##_##NSV;
            SA0_TABLE(X)
#undef X
            if (M.variant[p] < 0) return PRCNN_EUNSUPPORTED;
        }
        // every problem keeps its own (persistent) grid: the dense lists' bounds are 4-8 x the flat lists' and usually empty, so a
        // division of the resident slots by row bound would hand most of them to workgroups that leave at once
        const long grid = level_units_share(M.U, want, nullptr, n, 0);
        if (grid <= 0) return prcnn_fail(PRCNN_EINVAL, "prcnn_mlp_chain_group_multi: bad grid");
        hipLaunchKernelGGL(sa0_multi_kernel, dim3((unsigned)grid), dim3(256), 0, s, M);
        PRCNN_LAUNCH_CHECK("prcnn_mlp_chain_group_multi(sa0)");
        return PRCNN_OK;
    }
    // the other two families: two instantiated bodies, the wider one variant 0
    int va = 0, vb = 1 << 30;
    for (int p = 0; p < n; p++) {
        if (family == K_CHAIN_FAST && (L[p].b != 4 || L[p].c != 0)) return PRCNN_EUNSUPPORTED;
        va = max(va, L[p].a);
        vb = min(vb, L[p].a);
    }
    for (int p = 0; p < n; p++) {
        if (L[p].a != va && L[p].a != vb) return PRCNN_EUNSUPPORTED;
        M.variant[p] = L[p].a == va ? 0 : 1;
    }
    if (family == K_CHAIN_FAST) {
        const long grid = level_units_share(M.U, want, nullptr, n, 0);
        if (grid <= 0) return prcnn_fail(PRCNN_EINVAL, "prcnn_mlp_chain_group_multi: bad grid");
#define X(A, B)                                                                                                          \
        if (va == A && vb == B) {                                                                                        \
            hipLaunchKernelGGL((chain_fast_multi_kernel<A, B>), dim3((unsigned)grid), dim3(256), 0, s, M);               \
            PRCNN_LAUNCH_CHECK("prcnn_mlp_chain_group_multi(fast)");                                                     \
            return PRCNN_OK;                                                                                             \
        }
        FAST_MULTI_TABLE(X)
#undef X
        return PRCNN_EUNSUPPORTED;
    }
    size_t lds = 0;
    for (int p = 0; p < n; p++) lds = max(lds, L[p].lds);
    // the workgroups of the launch, at most the single launch's cap, in proportion to the problems' own (bounded) grids
    const long grid = level_units_share(M.U, want, nullptr, n, STACK_MULTI_GRID_CAP);
    if (grid <= 0) return prcnn_fail(PRCNN_EINVAL, "prcnn_mlp_chain_group_multi: bad grid");
#define X(A, B)                                                                                                          \
    if (va == A && vb == B) {                                                                                            \
        static PrcnnLdsLimit attr;                                                                                       \
        if (!attr.raise((const void*)stack2_multi_kernel<A, B>, 96 * 1024))                                              \
            return prcnn_fail(PRCNN_EHIP, "prcnn_mlp_chain_group_multi(stack): cannot raise the dynamic LDS limit");     \
        hipLaunchKernelGGL((stack2_multi_kernel<A, B>), dim3((unsigned)grid), dim3(256), lds, s, M);                     \
        PRCNN_LAUNCH_CHECK("prcnn_mlp_chain_group_multi(stack)");                                                        \
        return PRCNN_OK;                                                                                                 \
    }
    STACK_MULTI_TABLE(X)
#undef X
    return PRCNN_EUNSUPPORTED;
}

PRCNN_API int prcnn_mlp_chain_group_multi(int nprob, const prcnn_chain_group_problem_t* prob, prcnn_stream_t stream) {
    return chain_group_multi(nprob, prob, nullptr, nullptr, 0, nullptr, stream);
}

// ... storing by destination: dst[q] (host array over the problems, entries may be NULL) names where problem q's results go in
// the level output out2 (ld_out2 floats per row, problem q's columns at col_off2[q]) -- for an un-pooled problem per flat row
// (MlpParams::row_dst: prcnn_group_compact_pair_dst's rdst), for a pooled one per group (MlpParams::grp_dst: the dense list's
// listn).  Same kernels, grids and arithmetic; only the address of a stored row changes.
PRCNN_API int prcnn_mlp_chain_group_multi_dst(int nprob, const prcnn_chain_group_problem_t* prob, const int32_t* const* dst, float* out2,
                                              int ld_out2, const int* col_off2, prcnn_stream_t stream) {
    return chain_group_multi(nprob, prob, dst, out2, ld_out2, col_off2, stream);
}
