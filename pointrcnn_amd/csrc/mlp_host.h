// mlp_host.h -- the host front-end of mlp.hip: parameter fills, launch decisions, the one place that launches, the exports.
// Included once, at the bottom of mlp.hip (the kernels and MlpParams / ChainParams are above it; this is not a unit of its own).
//
//   1. fills      one function per operand mode writes MlpParams; layer exports, chain exports (through C.a) and the split
//                 chain exports share them
//   2. instances  the chain-instance table, and MlpLaunch: what a launcher decided (kernel instance, grid, block, dynamic LDS)
//   3. decide     decide_layer / decide_chain / decide_chain_split read switches and params only: no HIP call
//   4. launch     mlp_launch maps an MlpLaunch to its hipLaunchKernelGGL (and raises the LDS limit where the kernel needs it)
//   5. exports
//
// The ORDER in which mlp_launch names the kernel instances is the order they are instantiated in, and that is the order of the
// functions in the gfx950 code object: a reordered case gives the same ISA at other offsets.  Instances launched through a
// function template (launch_chain, launch_chain_fast, launch_chain_p) are instantiated at the end of the unit, after
// mlp_train.h's; that is why those three wrappers exist.
#pragma once

// ---- 1. fills ---------------------------------------------------------------------------------------
static void fill_out(MlpParams& P, const float* wpack, const float* bias, int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns) {
    P.wpack = wpack; P.bias = bias; P.Nout = Nout; P.relu = relu;
    P.out = out; P.ld_out = ld_out; P.col_off = col_off; P.pool_ns = pool_ns;
}

static void fill_plain(MlpParams& P, const float* in, int ld_in, long rows, int K) {
    P.rows = rows; P.K = K; P.in = in; P.ld_in = ld_in;
    P.vec_a = aligned16(in) && (ld_in % 4 == 0);
}

// act_wx / act_bias non-null: hoisted first layer -- feat_cl is Z = W_f . feat per source point (C = width of that
// layer), the A row is relu(Z[idx] + act_wx . dxyz + act_bias) and K = C.
// (the messages carry prcnn_mlp_group's name for every caller, as they always have)
static int fill_group(MlpParams& P, const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl, int ld_feat, int B, int N,
                      int M, int nsample, int C, const float* act_wx, const float* act_bias, const int32_t* groups_dev) {
    P.rows = (long)B * M * nsample; P.K = C + 3;
    P.rows_dev = groups_dev; P.rows_unit = nsample;
    P.xyz = xyz; P.new_xyz = new_xyz; P.idx = idx; P.feat = feat_cl; P.ld_feat = ld_feat;
    P.N = N; P.M = M; P.ns = nsample; P.C = C;
    P.vec_a = C > 0 && aligned16(feat_cl) && (ld_feat % 4 == 0);
    if (!act_wx && !act_bias) return PRCNN_OK;
    PRCNN_REQUIRE(act_wx && act_bias && C > 0, "prcnn_mlp_group: act_wx and act_bias must both be given (C > 0)");
    PRCNN_REQUIRE(aligned16(act_wx) && aligned16(act_bias) && C % 4 == 0,
                  "prcnn_mlp_group: hoisted mode needs 16-byte aligned act_wx/act_bias and C %% 4 == 0 (C=%d)", C);
    P.act = 1; P.act_wx = act_wx; P.act_bias = act_bias; P.K = C;
    return PRCNN_OK;
}

// act_bias non-null (requires C1 == 0): hoisted first layer -- known_cl is Y = W . known per known point, the A row
// is relu(interp(Y) + act_bias).  xcd_order: the chains' XCD-aware tile order (MlpParams::xcd_tpf), where the shape allows it.
// (the messages carry prcnn_mlp_interp's name for every caller, as they always have)
static int fill_interp(MlpParams& P, const float* known_cl, int ld_known, const int32_t* idx3, const float* w3, const float* skip_cl, int ld_skip,
                       int B, int n, int m, int C2, int C1, const float* act_bias, bool xcd_order) {
    P.rows = (long)B * n; P.K = C2 + C1;
    P.known = known_cl; P.idx3 = idx3; P.w3 = w3; P.skip = skip_cl; P.ld_known = ld_known; P.ld_skip = ld_skip;
    P.n = n; P.m = m; P.C2 = C2; P.C1 = C1;
    P.vec_a = aligned16(known_cl) && (ld_known % 4 == 0);
    P.vec_b = C1 > 0 && aligned16(skip_cl) && (ld_skip % 4 == 0) && (C2 % 4 == 0);
    if (act_bias) {
        PRCNN_REQUIRE(C1 == 0 && aligned16(act_bias) && C2 % 4 == 0,
                      "prcnn_mlp_interp: hoisted mode needs C1 == 0, aligned act_bias and C2 %% 4 == 0 (C2=%d C1=%d)", C2, C1);
        P.act = 2; P.act_bias = act_bias;
    }
    if (xcd_order && B % 8 == 0 && n % 128 == 0 && !sw_present(SW_NO_XCD_ORDER)) P.xcd_tpf = n / 128;
    return PRCNN_OK;
}

static int fill_chain(ChainParams& C, int nlayers, const float* const* wpack, const float* const* bias, const int* nout,
                      const int* relu, float* out, int ld_out, int col_off, int pool_ns) {
    PRCNN_REQUIRE(nlayers >= 1 && nlayers <= 3, "prcnn_mlp_chain: nlayers=%d (1..3)", nlayers);
    PRCNN_REQUIRE(wpack && bias && nout && relu && out, "prcnn_mlp_chain: null pointer");
    for (int l = 0; l < nlayers; l++) {
        PRCNN_REQUIRE(wpack[l] && aligned16(wpack[l]), "prcnn_mlp_chain: layer %d wpack null/unaligned", l);
        PRCNN_REQUIRE(bias[l] == nullptr || aligned16(bias[l]), "prcnn_mlp_chain: layer %d bias must be 16-byte aligned and padded to a multiple of 32", l);
        PRCNN_REQUIRE(nout[l] > 0 && nout[l] <= 512, "prcnn_mlp_chain: layer %d width %d (1..512)", l, nout[l]);
    }
    PRCNN_REQUIRE(pool_ns == 0 || pool_ns == 16 || pool_ns == 32, "prcnn_mlp_chain: pool_ns=%d (0/16/32)", pool_ns);
    PRCNN_REQUIRE(ld_out >= col_off + nout[nlayers - 1], "prcnn_mlp_chain: ld_out too small");
    C.nlayers = nlayers;
    fill_out(C.a, wpack[0], bias[0], nout[0], relu[0], out, ld_out, col_off, pool_ns);
    if (nlayers > 1) { C.wpack1 = wpack[1]; C.bias1 = bias[1]; C.N1 = nout[1]; C.relu1 = relu[1]; }
    if (nlayers > 2) { C.wpack2 = wpack[2]; C.bias2 = bias[2]; C.N2 = nout[2]; C.relu2 = relu[2]; }
    return PRCNN_OK;
}

// ---- 2. instances -----------------------------------------------------------------------------------
// The register-chain instances: X(mode, n0, n1, n2, PERS, KB0) -- widths in 32-column blocks (0: no such layer); PERS_KB with
// the KB of layer 0 where mlp_chain_pers_kernel has the instance too, PERS_NONE where it has not.  chain_instance_exists,
// prcnn_mlp_chain_supported, decide_chain and the generic and persistent launch cases all come from this table.
#define CHAIN_TABLE(X)                                                                                                 \
    X(MODE_GROUP, 1, 1, 1, PERS_NONE, 0) X(MODE_GROUP, 1, 1, 2, PERS_NONE, 0) X(MODE_GROUP, 2, 2, 4, PERS_NONE, 0) X(MODE_GROUP, 2, 3, 4, PERS_NONE, 0) \
    X(MODE_GROUP, 2, 4, 0, PERS_KB, 8) X(MODE_GROUP, 3, 4, 0, PERS_KB, 8)                   /* hoisted SA2 stacks */      \
    X(MODE_INTERP, 4, 4, 0, PERS_NONE, 0) X(MODE_INTERP, 4, 0, 0, PERS_KB, 16)              /* FP0 / hoisted FP0 */        \
    X(MODE_PLAIN, 4, 4, 0, PERS_NONE, 0) X(MODE_PLAIN, 4, 1, 0, PERS_KB, 16) X(MODE_PLAIN, 4, 3, 0, PERS_KB, 16)
// The rows that mlp_chain_fast_kernel has too.  A list of its own, because it cannot be a column: the fast kernels sit in the
// code object in THIS order (plain 4,4,0 last), the generic ones in the table's (plain 4,4,0 first), and one list has one order.
// chain_has_fast refuses at compile time a row that the table lacks.
#define CHAIN_FAST_TABLE(X) \
    X(MODE_GROUP, 2, 4, 0) X(MODE_GROUP, 3, 4, 0) X(MODE_INTERP, 4, 0, 0) X(MODE_PLAIN, 4, 1, 0) X(MODE_PLAIN, 4, 3, 0) X(MODE_PLAIN, 4, 4, 0)
// SA level 0 (sa_xyz_chain_kernel): X(width of layer 0, of layer 1, n2, nsample)
#define SA0_TABLE(X) X(16, 16, 1, 16) X(32, 32, 2, 32) X(16, 16, 1, 1) X(32, 32, 2, 1)

static constexpr bool chain_instance_exists(int mode, int n0, int n1, int n2) {
#define X(M, A, B, CC, PERS, KB0V) if (mode == M && n0 == A && n1 == B && n2 == CC) return true;
    CHAIN_TABLE(X)
#undef X
    return false;
}
static bool chain_has_fast(int mode, int n0, int n1, int n2) {
#define X(M, A, B, CC) static_assert(chain_instance_exists(M, A, B, CC), "a fast chain instance that the chain table lacks"); \
    if (mode == M && n0 == A && n1 == B && n2 == CC) return true;
    CHAIN_FAST_TABLE(X)
#undef X
    return false;
}

enum MlpFamily { K_NONE, K_LAYER_S, K_LAYER_B, K_LAYER_V1, K_ROWS32, K_CHAIN_S, K_CHAIN_C, K_CHAIN_P, K_STACK2, K_SA0, K_CHAIN_PERS, K_CHAIN_FAST, K_CHAIN };
// What a launcher decided.  K_NONE: nothing to launch (no rows).  a..d are the family's template arguments after the mode:
//   K_LAYER_S  WNB, TERMS, ADDY, LOOP      K_LAYER_B  WNB, FAST, ADDY      K_LAYER_V1  WNB      K_ROWS32  a = split_max (an argument)
//   K_CHAIN_S / _C  NB1, TERMS             K_CHAIN_P  NB1 (its grid follows the device's CU count: launch_chain_p)
//   K_STACK2  NBW0      K_SA0  KB1, KB2, NB2, NS      K_CHAIN_PERS  NB0, NB1, NB2, KB0      K_CHAIN_FAST / K_CHAIN  NB0, NB1, NB2
struct MlpLaunch {
    int family = K_NONE, mode = 0, a = 0, b = 0, c = 0, d = 0;
    dim3 grid, block;
    size_t lds = 0;
    const char* what = "";       // names the launch in a launch-failure message
    void set(int family_, int mode_, int a_, int b_, int c_, int d_, dim3 grid_, dim3 block_, size_t lds_, const char* what_) {
        family = family_; mode = mode_; a = a_; b = b_; c = c_; d = d_; grid = grid_; block = block_; lds = lds_; what = what_;
    }
};

// ---- 3. decide --------------------------------------------------------------------------------------
static int nb32(int n) { return (n + 31) / 32; }

// PRCNN_CHAIN_PERSIST=0: the per-tile kernels (A/B switch, same bits)
static bool chain_persist_on() { return sw_enabled(SW_CHAIN_PERSIST); }
static bool chain_coop_on() { return sw_num(SW_CHAIN_COOP, 1) != 0; }
static bool chain_coop_forced() { return sw_num(SW_CHAIN_COOP, 1) == 2; }      // 2: the cooperative form also where the lane-is-a-row kernel is the default

static bool rows32_ok(int mode, const MlpParams& P) {
    return !sw_present(SW_NO_ROWS32) && mode == MODE_PLAIN && !P.addY && P.pool_ns == 0 && !P.seg_cnt && P.vec_a && P.K % 8 == 0 && P.K >= 256 &&
           P.K <= R32_MAX_K && P.Nout >= 128 && P.rows <= 4096;
}

// one layer: checks the params, writes KB / NB / wgm_cols
static int decide_layer(int mode, MlpParams& P, MlpLaunch& L) {
    PRCNN_REQUIRE(P.wpack && P.out, "prcnn_mlp: null weight/output pointer");
    PRCNN_REQUIRE(P.rows >= 0 && P.K > 0 && P.Nout > 0, "prcnn_mlp: bad shape rows=%ld K=%d Nout=%d", P.rows, P.K, P.Nout);
    PRCNN_REQUIRE(P.pool_ns == 0 || P.pool_ns == 16 || P.pool_ns == 32 || P.pool_ns == 64,
                  "prcnn_mlp: pool_ns=%d unsupported (use 16/32/64, or store + prcnn_maxpool_rows)", P.pool_ns);
    PRCNN_REQUIRE(P.pool_ns == 0 || P.rows % P.pool_ns == 0, "prcnn_mlp: rows %ld not a multiple of pool_ns %d", P.rows, P.pool_ns);
    PRCNN_REQUIRE(aligned16(P.wpack), "prcnn_mlp: wpack must be 16-byte aligned");
    if (P.rows == 0) return PRCNN_OK;
    P.KB = (P.K + 7) / 8;
    P.NB = (P.Nout + 31) / 32;
    const int row_tiles = prcnn_divup(P.rows, MLP_BM);
    // split-bf16 variant: 128 x 128 tiles while they give most CUs a workgroup (two are resident per CU), else 128 x 64.  Every
    // launch of a supported shape takes it, however few its rows: which arithmetic a layer is computed in must not depend on the
    // batch size (a frame's result is the same bits in a batch of 1 and of 32).  PRCNN_SPLIT_MIN_TILES (dev A/B) sends launches of
    // fewer tiles to the fp32 kernels, which have forms for few rows.
    const long tiles_wide = (long)row_tiles * prcnn_divup(P.NB, 4), tiles_narrow = (long)row_tiles * prcnn_divup(P.NB, 2);
    // the hoisted grouped form (prcnn_mlp_group_split); PRCNN_GROUP_SPLIT=0: A/B switch back to the fp32 layer kernel
    const bool split_group = sw_enabled(SW_GROUP_SPLIT) && mode == MODE_GROUP && P.act == 1 && P.C == P.K && !P.addY;
    if (P.wsplit && (mode == MODE_PLAIN || split_group) && P.K % MLP_BK == 0 && P.vec_a && tiles_narrow >= sw_num(SW_SPLIT_MIN_TILES, 0)) {
        PRCNN_REQUIRE(aligned16(P.wsplit) && (P.split_terms == 3 || P.split_terms == 6), "prcnn_mlp: bad split image / terms=%d", P.split_terms);
        const bool wide = P.NB >= 4 && tiles_wide >= sw_num(SW_SPLIT_WIDE_MIN, 192);
        dim3 grid(row_tiles, prcnn_divup(P.NB, wide ? 4 : 2));
        if (!P.seg_cnt) {
            P.wgm_cols = (int)grid.y;
            grid = dim3((unsigned)(prcnn_divup(grid.x, 8) * 8 * grid.y), 1);
        }
        // a launch sized for the CAPACITY of a compacted list (device-side row count): 2048 workgroups (four rounds of the 512 resident
        // ones, a multiple of the 8 XCDs) walk the live tiles instead of one workgroup per tile of capacity; PRCNN_BOUNDED_GRID=0: A/B
        const bool bounded = sw_enabled(SW_BOUNDED_GRID) && P.rows_dev && !P.seg_cnt && !P.addY && grid.x > 2048u;
        if (bounded) grid = dim3(2048u, 1);
        // (the addend form is plain rows and never bounded; the grouped form has no addend)
        L.set(K_LAYER_S, mode, wide ? 2 : 1, P.split_terms, P.addY != nullptr, bounded, grid, dim3(MLP_THREADS), 0, "prcnn_mlp (split-bf16)");
        return PRCNN_OK;
    }
    if (rows32_ok(mode, P)) {
        const int split_max = prcnn_divup(P.NB, 4);
        L.set(K_ROWS32, mode, split_max, 0, 0, 0, dim3((unsigned)min((long)prcnn_divup(P.rows, ST_ROWS) * split_max, 2048L)), dim3(256),
              (size_t)ST_ROWS * (P.K + 4) * sizeof(float), "prcnn_mlp(rows32)");
        return PRCNN_OK;
    }
    // >= 97 output channels: 128x128 workgroup tile -- unless that leaves most of the 256 CUs without a workgroup
    // (few rows, e.g. FP3's 2048 known points): then the 128x64 tile doubles the number of workgroups
    // (a device-side row count means a compacted list: P.rows is its worst case, the live part is expected to be small)
    bool wide = P.NB >= 4 && (!P.rows_dev || sw_present(SW_WIDE_LISTS)) && tiles_wide >= sw_num(SW_WIDE_MIN_TILES, 192);
    // v2 (B operand straight from L2, up to four workgroups per CU) is the default; PRCNN_LAYER_V1=1 is the A/B switch (same bits).
    const bool v2 = !sw_present(SW_LAYER_V1);
    // (fast = straight-line main loop, see mlp_layer_b_kernel: whole 32-wide chunks, 16-byte rows; grouped: the hoisted form only)
    const bool fast = P.K % MLP_BK == 0 && P.vec_a && (mode == MODE_PLAIN || (mode == MODE_GROUP && P.act == 1 && P.C == P.K));
    if (v2 && fast && mode == MODE_PLAIN && wide && !sw_present(SW_WIDE_MIN_TILES)) {
        // four workgroups per CU = 1024 resident tiles: with >= 1024 wide tiles the narrow tile (twice as many, half as long)
        // runs in more, staggered rounds, so one round's store epilogue overlaps the next one's main loop (measured: 32768 x
        // 512 -> 512 171 -> 160 us, 131072 x 256 -> 256 173 -> 167 us); between 384 and 1023 wide tiles the wide tile's better
        // MFMA : LDS-read ratio wins (32768 x 512 -> 256: 74 vs 81 us)
        wide = tiles_wide >= 384 && tiles_wide < 1024;
    }
    dim3 grid(row_tiles, prcnn_divup(P.NB, wide ? 4 : 2));
    if (v2 && mode == MODE_PLAIN && !P.seg_cnt && P.xcd_tpf == 0 && !sw_present(SW_NO_WGM)) {
        P.wgm_cols = (int)grid.y;
        grid = dim3((unsigned)(prcnn_divup(grid.x, 8) * 8 * grid.y), 1);
    }
    if (v2) L.set(K_LAYER_B, mode, wide ? 2 : 1, fast, mode == MODE_PLAIN && P.addY, 0, grid, dim3(MLP_THREADS), 0, "prcnn_mlp");
    else L.set(K_LAYER_V1, mode, wide ? 2 : 1, 0, 0, 0, grid, dim3(MLP_THREADS), 0, "prcnn_mlp");
    return PRCNN_OK;
}

// the straight-line variant applies when nothing in the layer-0 loop needs a bounds check (see mlp_chain_fast_kernel)
static bool chain_fast_ok(int mode, const ChainParams& C, int n0, int n1, int n2) {
    const MlpParams& P = C.a;
    if (P.K % 8 != 0 || P.K > FAST_MAX_K || P.K < 16 || !P.vec_a || P.addY) return false;
    const int G0 = n0 == 3 ? 4 : CH_STAGE_TILES / n0;
    if ((P.K / 8) % G0 != 0) return false;
    if (n1 > 0 && P.Nout != n0 * 32) return false;                 // KB of layer 1 == 4 * NB0
    if (n2 > 0 && C.N1 != n1 * 32) return false;
    if (n1 > 0 && (n0 * 4) % (n1 == 3 ? 4 : CH_STAGE_TILES / n1) != 0) return false;
    if (n2 > 0 && (n1 * 4) % (n2 == 3 ? 4 : CH_STAGE_TILES / n2) != 0) return false;
    if (mode == MODE_GROUP) return P.act == 1 && P.K == P.C && P.act_wx && P.act_bias;
    if (mode == MODE_INTERP) return P.act == 2 && P.C1 == 0 && P.K == P.C2 && P.act_bias;
    return mode == MODE_PLAIN;
}

// shapes the stack kernel takes (hoisted grouped form on flat row lists, no pooling)
static bool stack2_ok(int mode, const ChainParams& C) {
    const MlpParams& P = C.a;
    return mode == MODE_GROUP && C.nlayers == 2 && P.act == 1 && P.pool_ns == 0 && P.ns == 1 && P.C == P.K && P.K % 8 == 0 &&
           P.K <= ST_MAX_K0 && P.vec_a && (P.Nout > 128 || C.N1 > 128) && nb32(P.Nout) <= ST_MAX_NB0 && nb32(C.N1) <= 16;
}

// a fp32 chain: writes KB / NB / KB1 / KB2 / stack_split; PRCNN_EUNSUPPORTED when no instance matches
static int decide_chain(int mode, ChainParams& C, MlpLaunch& L) {
    MlpParams& P = C.a;
    P.KB = (P.K + 7) / 8;
    P.NB = nb32(P.Nout);
    const int n0 = nb32(P.Nout), n1 = C.nlayers > 1 ? nb32(C.N1) : 0, n2 = C.nlayers > 2 ? nb32(C.N2) : 0;
    if (C.nlayers > 1) C.KB1 = (P.Nout + 7) / 8;
    if (C.nlayers > 2) C.KB2 = (C.N1 + 7) / 8;
    if (P.rows == 0) return PRCNN_OK;
    const dim3 tiles128(prcnn_divup(P.rows, 128));
    if (stack2_ok(mode, C)) {
        // stack_split = the most workgroups a row tile's layer-B column groups may be dealt to; the kernel picks the split
        // from the device-side row count
        const int nbw0 = prcnn_divup(n0, 4);
        C.stack_split = prcnn_divup(n1, 4);
        if (nbw0 >= 1 && nbw0 <= 3) {
            L.set(K_STACK2, mode, nbw0, 0, 0, 0, dim3((unsigned)min((long)prcnn_divup(P.rows, ST_ROWS) * C.stack_split, 2048L)), dim3(256),
                  (size_t)ST_ROWS * ((P.K + 4) + (nb32(P.Nout) * 32 + 4)) * sizeof(float), "prcnn_mlp_chain(stack)");
            return PRCNN_OK;
        }
    }
    // SA level 0: xyz-only rows, three narrow layers, pooled -- persistent register-weight kernel
    // (pooled groups, or -- nsample 1, no pooling -- the flat row list of the padding-free path: the same kernel writes rows)
    if (mode == MODE_GROUP && P.C == 0 && !P.act && P.K == 3 && C.nlayers == 3 && P.new_xyz &&
        (P.pool_ns == P.ns || (P.pool_ns == 0 && P.ns == 1)) && C.N2 % 4 == 0 &&
        !sw_present(SW_NO_SA0)) {              // (A/B switch; the generic chain kernel gives the same bits)
        // persistent: one resident workgroup per occupancy slot (256 CUs x 3 or 2 workgroups at 115 / 243 registers)
#define X(W0, W1, NBL, NSV)                                                                                                              \
        if (P.Nout == W0 && C.N1 == W1 && n2 == NBL && P.ns == NSV) {                                                                    \
            L.set(K_SA0, mode, W0 / 8, W1 / 8, NBL, NSV, dim3((int)min((long)(NBL == 1 ? 768 : 512), (long)prcnn_divup(P.rows, 128))), dim3(256), 0, \
                  "prcnn_mlp_chain(sa0)");                                                                                               \
            return PRCNN_OK;                                                                                                             \
        }
        SA0_TABLE(X)
#undef X
    }
    // Opt-in (PRCNN_PERSISTENT_CHAIN=1): 6-12 % faster per launch with ONE batch in flight, but a persistent workgroup
    // holds its CU's LDS for the whole kernel, which starves the other in-flight batches' kernels (FPS sort, layer tiles):
    // measured -6 % RPN throughput at 3 batches in flight, so the default keeps the per-tile workgroups.
    if (chain_fast_ok(mode, C, n0, n1, n2) && !P.seg_cnt && sw_present(SW_PERSISTENT_CHAIN)) {
        // persistent form: weights of the whole stack resident in LDS, one 8-wave workgroup per CU
#define PERS_NONE(M, KB0V, A, B, CC)
#define PERS_KB(M, KB0V, A, B, CC)                                                                                                       \
        if (mode == M && P.KB == KB0V && n0 == A && n1 == B && n2 == CC) {                                                               \
            L.set(K_CHAIN_PERS, mode, A, B, CC, KB0V, dim3((int)min((long)256, (long)prcnn_divup(P.rows, 32 * PERS_WAVES))), dim3(PERS_WAVES * 64), \
                  pers_lds_bytes<M, KB0V, A, B, CC>(), "prcnn_mlp_chain(persistent)");                                                   \
            return PRCNN_OK;                                                                                                             \
        }
#define X(M, A, B, CC, PERS, KB0V) PERS(M, KB0V, A, B, CC)
        CHAIN_TABLE(X)
#undef X
#undef PERS_KB
#undef PERS_NONE
    }
    if (chain_fast_ok(mode, C, n0, n1, n2) && !sw_present(SW_NO_FAST_CHAIN) && chain_has_fast(mode, n0, n1, n2)) {      // (A/B switch, same bits)
        L.set(K_CHAIN_FAST, mode, n0, n1, n2, 0, tiles128, dim3(256), 0, "prcnn_mlp_chain(fast)");
        return PRCNN_OK;
    }
    if (chain_instance_exists(mode, n0, n1, n2)) {
        L.set(K_CHAIN, mode, n0, n1, n2, 0, tiles128, dim3(256), 0, "prcnn_mlp_chain");
        return PRCNN_OK;
    }
    return prcnn_fail(PRCNN_EUNSUPPORTED, "prcnn_mlp_chain: no register-chain instance for mode %d widths (%d,%d,%d)/32", mode, n0, n1, n2);
}

// a split-bf16 chain (prcnn_mlp_chain_rows_split: plain rows, nb1 = 1 / 3 / 4; prcnn_mlp_chain_interp_split: nb1 = 0).
// pers_fits: the persistent kernel's 32-bit row offsets (in floats) reach every source row; it has the instances <plain, 1> and <interp, 0>.
// Plain rows, two layers: the lane-is-a-row kernel stays the default (its 32 rows are 16 contiguous KB that the 16 k-steps
// re-read from L1: 168 vs 179 us for the reg head); PRCNN_CHAIN_COOP=2 selects the cooperative form (same bits).
static void decide_chain_split(int mode, int nb1, int terms, bool pers_fits, long rows, const char* what, MlpLaunch& L) {
    const bool coop = mode == MODE_PLAIN ? chain_coop_forced() : chain_coop_on();
    const int family = nb1 <= 1 && terms == 6 && chain_coop_on() && chain_persist_on() && pers_fits ? K_CHAIN_P
                       : terms == 6 && coop                                                         ? K_CHAIN_C
                                                                                                    : K_CHAIN_S;
    L.set(family, mode, nb1, family == K_CHAIN_S ? terms : 6, 0, 0, dim3(prcnn_divup(rows, 128)), dim3(256), 0, what);
}

// ---- 4. launch --------------------------------------------------------------------------------------
template <int MODE, int NB0, int NB1, int NB2>
static void launch_chain(const MlpLaunch& L, const ChainParams& C, hipStream_t s) {
    hipLaunchKernelGGL((mlp_chain_kernel<MODE, NB0, NB1, NB2>), L.grid, L.block, L.lds, s, C);
}
template <int MODE, int NB0, int NB1, int NB2>
static void launch_chain_fast(const MlpLaunch& L, const ChainParams& C, hipStream_t s) {
    hipLaunchKernelGGL((mlp_chain_fast_kernel<MODE, NB0, NB1, NB2>), L.grid, L.block, L.lds, s, C);
}
static int chain_p_grid() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        return n & ~7;                                        // a multiple of 8: the XCD-aware tile order counts on it
    }();
    return cus > 0 ? cus : 8;
}
template <int MODE, int NB1>
static int launch_chain_p(const ChainParams& C, hipStream_t s) {
    constexpr size_t lds = chain_p_lds_bytes<MODE, NB1>();
    static PrcnnLdsLimit attr;
    if (!attr.raise((const void*)mlp_chain_p_kernel<MODE, NB1, 6>, (int)lds))
        return prcnn_fail(PRCNN_EHIP, "prcnn_mlp_chain(persistent split): cannot raise the dynamic LDS limit");
    const long tiles = (C.a.rows + 31) / 32;
    const int grid = (int)min((long)chain_p_grid(), (tiles + CP_WAVES - 1) / CP_WAVES);
    hipLaunchKernelGGL((mlp_chain_p_kernel<MODE, NB1, 6>), dim3(grid), dim3(CP_WAVES * 64), lds, s, C);
    return PRCNN_OK;
}

// The one place that launches.  P: the layer kernels' argument; C: the chain kernels' (null for a layer).  Keep the order of the cases.
static int mlp_launch(const MlpLaunch& L, const MlpParams& P, const ChainParams* C, hipStream_t s) {
    if (L.family == K_NONE) return PRCNN_OK;
#define IS(F, M, A, B, CC, D) (L.family == F && L.mode == M && L.a == A && L.b == B && L.c == CC && L.d == D)
#define GO(kernel, ...) hipLaunchKernelGGL(kernel, L.grid, L.block, L.lds, s, __VA_ARGS__)
#define RAISE(kernel, bytes, who)                                                                           \
    static PrcnnLdsLimit attr;                                                                              \
    if (!attr.raise((const void*)kernel, (int)(bytes))) return prcnn_fail(PRCNN_EHIP, who ": cannot raise the dynamic LDS limit")
    // split-bf16 layer: grouped (bounded grid or not), plain with the addend, plain (bounded grid or not)
#define S_CASE(M, W, T, ADDY, LOOP) if (IS(K_LAYER_S, M, W, T, ADDY, LOOP)) GO((mlp_layer_s_kernel<M, W, T, ADDY, LOOP>), P); else
#define S_FORMS(W, T) S_CASE(MODE_GROUP, W, T, false, true) S_CASE(MODE_GROUP, W, T, false, false) S_CASE(MODE_PLAIN, W, T, true, false) \
                      S_CASE(MODE_PLAIN, W, T, false, true) S_CASE(MODE_PLAIN, W, T, false, false)
    S_FORMS(2, 6) S_FORMS(2, 3) S_FORMS(1, 6) S_FORMS(1, 3)
    // fp32 layer, v2 and v1: per mode the fast forms (wide, narrow), the general ones, v1; only plain rows have the addend
#define B_CASE(M, W, F, ADDY) if (IS(K_LAYER_B, M, W, F, ADDY, 0)) GO((mlp_layer_b_kernel<M, W, F, ADDY>), P); else
#define V1_CASE(M, W) if (IS(K_LAYER_V1, M, W, 0, 0, 0)) GO((mlp_layer_kernel<M, W>), P); else
    B_CASE(MODE_PLAIN, 2, true, true) B_CASE(MODE_PLAIN, 2, true, false) B_CASE(MODE_PLAIN, 1, true, true) B_CASE(MODE_PLAIN, 1, true, false)
    B_CASE(MODE_PLAIN, 2, false, true) B_CASE(MODE_PLAIN, 2, false, false) B_CASE(MODE_PLAIN, 1, false, true) B_CASE(MODE_PLAIN, 1, false, false)
    V1_CASE(MODE_PLAIN, 2) V1_CASE(MODE_PLAIN, 1)
    B_CASE(MODE_GROUP, 2, true, false) B_CASE(MODE_GROUP, 1, true, false) B_CASE(MODE_GROUP, 2, false, false) B_CASE(MODE_GROUP, 1, false, false)
    V1_CASE(MODE_GROUP, 2) V1_CASE(MODE_GROUP, 1)
    B_CASE(MODE_INTERP, 2, false, false) B_CASE(MODE_INTERP, 1, false, false) V1_CASE(MODE_INTERP, 2) V1_CASE(MODE_INTERP, 1)
    if (L.family == K_ROWS32) {
        RAISE(mlp_rows32_kernel, 144 * 1024, "prcnn_mlp(rows32)");
        GO(mlp_rows32_kernel, P, L.a);
    } else
    // split-bf16 chains: persistent, cooperative, lane-is-a-row (six terms, three terms)
#define P_CASE(M, NB1) if (IS(K_CHAIN_P, M, NB1, 6, 0, 0)) { const int rc = launch_chain_p<M, NB1>(*C, s); if (rc) return rc; } else
#define SC_FORMS(M, NB1) if (IS(K_CHAIN_C, M, NB1, 6, 0, 0)) GO((mlp_chain_c_kernel<M, NB1, 6>), *C); else \
                         if (IS(K_CHAIN_S, M, NB1, 6, 0, 0)) GO((mlp_chain_s_kernel<M, NB1, 6>), *C); else \
                         if (IS(K_CHAIN_S, M, NB1, 3, 0, 0)) GO((mlp_chain_s_kernel<M, NB1, 3>), *C); else
    P_CASE(MODE_PLAIN, 1) SC_FORMS(MODE_PLAIN, 1) SC_FORMS(MODE_PLAIN, 3) SC_FORMS(MODE_PLAIN, 4)
#define STACK_CASE(A) if (IS(K_STACK2, MODE_GROUP, A, 0, 0, 0)) { RAISE(mlp_stack2_kernel<A>, 96 * 1024, "prcnn_mlp_chain(stack)"); GO((mlp_stack2_kernel<A>), *C); } else
    STACK_CASE(1) STACK_CASE(2) STACK_CASE(3)
#define X(W0, W1, NBL, NSV) if (IS(K_SA0, MODE_GROUP, W0 / 8, W1 / 8, NBL, NSV)) GO((sa_xyz_chain_kernel<W0 / 8, W1 / 8, NBL, NSV>), *C); else
    SA0_TABLE(X)
#undef X
#define PERS_NONE(M, KB0V, A, B, CC)
#define PERS_KB(M, KB0V, A, B, CC)                                                                                                     \
    if (IS(K_CHAIN_PERS, M, A, B, CC, KB0V)) {                                                                                         \
        RAISE((mlp_chain_pers_kernel<M, KB0V, A, B, CC>), L.lds, "prcnn_mlp_chain");                                                   \
        GO((mlp_chain_pers_kernel<M, KB0V, A, B, CC>), *C);                                                                            \
    } else
#define X(M, A, B, CC, PERS, KB0V) PERS(M, KB0V, A, B, CC)
    CHAIN_TABLE(X)
#undef X
#define X(M, A, B, CC) if (IS(K_CHAIN_FAST, M, A, B, CC, 0)) launch_chain_fast<M, A, B, CC>(L, *C, s); else
    CHAIN_FAST_TABLE(X)
#undef X
#define X(M, A, B, CC, PERS, KB0V) if (IS(K_CHAIN, M, A, B, CC, 0)) launch_chain<M, A, B, CC>(L, *C, s); else
    CHAIN_TABLE(X)
#undef X
    P_CASE(MODE_INTERP, 0) SC_FORMS(MODE_INTERP, 0)
        return prcnn_fail(PRCNN_EINVAL, "prcnn_mlp: no kernel instance for family %d mode %d <%d,%d,%d,%d>", L.family, L.mode, L.a, L.b, L.c, L.d);
#undef PERS_KB
#undef PERS_NONE
#undef STACK_CASE
#undef SC_FORMS
#undef P_CASE
#undef V1_CASE
#undef B_CASE
#undef S_FORMS
#undef S_CASE
#undef RAISE
#undef GO
#undef IS
    PRCNN_LAUNCH_CHECK(L.what);
    return PRCNN_OK;
}

static int launch_mlp(int mode, MlpParams& P, hipStream_t s) {
    MlpLaunch L;
    const int rc = decide_layer(mode, P, L);
    return rc ? rc : mlp_launch(L, P, nullptr, s);
}
static int dispatch_chain(int mode, ChainParams& C, hipStream_t s) {
    MlpLaunch L;
    const int rc = decide_chain(mode, C, L);
    return rc ? rc : mlp_launch(L, C.a, &C, s);
}

// ---- 5. exports -------------------------------------------------------------------------------------
PRCNN_API size_t prcnn_wpack_floats(int Nout, int K) {
    if (Nout <= 0 || K <= 0) return 0;
    return (size_t)((Nout + 31) / 32) * ((K + 7) / 8) * 256;
}

PRCNN_API int prcnn_pack_weight(const float* w, int Nout, int K, int k_rot, float* wpack, prcnn_stream_t stream) {
    PRCNN_REQUIRE(w && wpack, "prcnn_pack_weight: null pointer");
    PRCNN_REQUIRE(Nout > 0 && K > 0 && k_rot >= 0 && k_rot <= K, "prcnn_pack_weight: bad shape Nout=%d K=%d k_rot=%d", Nout, K, k_rot);
    int KB = (K + 7) / 8, NB = (Nout + 31) / 32;
    long total = (long)NB * KB * 256;
    hipLaunchKernelGGL(pack_weight_kernel, dim3(prcnn_divup(total, 256)), dim3(256), 0, (hipStream_t)stream, w, Nout, K,
                       k_rot, KB, NB, wpack);
    PRCNN_LAUNCH_CHECK("prcnn_pack_weight");
    return PRCNN_OK;
}

PRCNN_API size_t prcnn_wsplit_bytes(int Nout, int K) {
    if (Nout <= 0 || K <= 0) return 0;
    // whole 32-wide chunks of k (two k-steps each): the training images of a ragged K are zero-padded that far; K % 32 == 0: (K + 15) / 16
    return (size_t)((Nout + 31) / 32) * (((K + 31) / 32) * 2) * 3 * 1024;
}

PRCNN_API int prcnn_pack_weight_split(const float* w, int Nout, int K, int chain, void* wsplit, prcnn_stream_t stream) {
    PRCNN_REQUIRE(w && wsplit && aligned16(wsplit), "prcnn_pack_weight_split: null / misaligned pointer");
    PRCNN_REQUIRE(Nout > 0 && K > 0 && (chain == 0 || chain == 1), "prcnn_pack_weight_split: bad shape Nout=%d K=%d chain=%d", Nout, K, chain);
    const int KS = (K + 15) / 16, NB = (Nout + 31) / 32;
    hipLaunchKernelGGL(pack_weight_split_kernel, dim3(prcnn_divup((long)NB * KS * 64, 256)), dim3(256), 0, (hipStream_t)stream, w,
                       Nout, K, KS, NB, chain, reinterpret_cast<uint4*>(wsplit));
    PRCNN_LAUNCH_CHECK("prcnn_pack_weight_split");
    return PRCNN_OK;
}

PRCNN_API int prcnn_maxpool_rows(const float* in, int ld_in, int64_t rows_out, int ns, int C, float* out, int ld_out,
                                 int col_off, prcnn_stream_t stream) {
    PRCNN_REQUIRE(in && out, "prcnn_maxpool_rows: null pointer");
    PRCNN_REQUIRE(rows_out >= 0 && ns > 0 && C > 0 && ld_in >= C && ld_out >= col_off + C, "prcnn_maxpool_rows: bad shape");
    if (rows_out == 0) return PRCNN_OK;
    hipLaunchKernelGGL(maxpool_rows_kernel, dim3(prcnn_divup(rows_out * C, 256)), dim3(256), 0, (hipStream_t)stream, in,
                       ld_in, (long)rows_out, ns, C, out, ld_out, col_off);
    PRCNN_LAUNCH_CHECK("prcnn_maxpool_rows");
    return PRCNN_OK;
}

// Every _split layer export is its fp32 twin plus the split image: one body each, `who` names the export in the messages and
// wsplit / terms are read only where split is set.
static int mlp_rows_body(const char* who, bool split, const float* in, int ld_in, int64_t rows, int K, const float* wpack, const void* wsplit,
                         int terms, const float* bias, int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns,
                         const int32_t* rows_dev, int rows_unit, const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream) {
    if (split) PRCNN_REQUIRE(in && wsplit, "%s: null pointer", who);
    else PRCNN_REQUIRE(in, "%s: null input", who);
    PRCNN_REQUIRE(ld_in >= K && ld_out >= col_off + Nout, "%s: bad strides ld_in=%d K=%d ld_out=%d", who, ld_in, K, ld_out);
    if (split) PRCNN_REQUIRE(terms == 3 || terms == 6, "%s: terms=%d (3 or 6)", who, terms);
    MlpParams P = {};
    fill_out(P, wpack, bias, Nout, relu, out, ld_out, col_off, pool_ns);
    fill_plain(P, in, ld_in, rows, K);
    P.rows_dev = rows_dev; P.rows_unit = rows_unit > 0 ? rows_unit : 1;
    PRCNN_REQUIRE(!seg_cnt || (seg_rows > 0 && seg_rows % MLP_BM == 0 && rows % seg_rows == 0 && pool_ns == 0 && !rows_dev),
                  "%s: seg_rows=%d must be a multiple of %d dividing rows (no pooling, no rows_dev)", who, seg_rows, MLP_BM);
    P.seg_cnt = seg_cnt; P.seg_rows = seg_rows;
    if (split) { P.wsplit = wsplit; P.split_terms = terms; }
    return launch_mlp(MODE_PLAIN, P, (hipStream_t)stream);
}

PRCNN_API int prcnn_mlp_rows(const float* in, int ld_in, int64_t rows, int K, const float* wpack, const float* bias,
                             int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns,
                             const int32_t* rows_dev, int rows_unit, const int32_t* seg_cnt, int seg_rows,
                             prcnn_stream_t stream) {
    return mlp_rows_body("prcnn_mlp_rows", false, in, ld_in, rows, K, wpack, nullptr, 0, bias, Nout, relu, out, ld_out, col_off, pool_ns, rows_dev,
                         rows_unit, seg_cnt, seg_rows, stream);
}

PRCNN_API int prcnn_mlp_rows_split(const float* in, int ld_in, int64_t rows, int K, const float* wpack, const void* wsplit, int terms,
                                   const float* bias, int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns,
                                   const int32_t* rows_dev, int rows_unit, const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream) {
    return mlp_rows_body("prcnn_mlp_rows_split", true, in, ld_in, rows, K, wpack, wsplit, terms, bias, Nout, relu, out, ld_out, col_off, pool_ns,
                         rows_dev, rows_unit, seg_cnt, seg_rows, stream);
}

static int mlp_rows_addinterp_body(const char* who, bool split, const float* in, int ld_in, int K, const float* wpack, const void* wsplit, int terms,
                                   const float* bias, int Nout, int relu, const float* y_cl, int ld_y, const int32_t* idx3, const float* w3,
                                   int B, int n, int m, float* out, int ld_out, int col_off, prcnn_stream_t stream) {
    PRCNN_REQUIRE(in && y_cl && idx3 && w3 && (!split || wsplit), "%s: null pointer", who);
    PRCNN_REQUIRE(B >= 0 && n > 0 && m > 0 && ld_in >= K && ld_y >= Nout && ld_out >= col_off + Nout,
                  "%s: bad shape B=%d n=%d m=%d K=%d Nout=%d", who, B, n, m, K, Nout);
    if (split) PRCNN_REQUIRE(terms == 3 || terms == 6, "%s: terms=%d (3 or 6)", who, terms);
    MlpParams P = {};
    fill_out(P, wpack, bias, Nout, relu, out, ld_out, col_off, 0);
    fill_plain(P, in, ld_in, (long)B * n, K);
    P.addY = y_cl; P.ldY = ld_y; P.idx3 = idx3; P.w3 = w3; P.n = n; P.m = m;
    P.addy_phase = (int)sw_num(SW_ADDY_PHASE, 2);      // A/B switch: 0 = all in the epilogue
    // (rows_unit is read only beside rows_dev, effective_rows(), and there is none here: the split export has always set it, its twin not)
    if (split) { P.rows_unit = 1; P.wsplit = wsplit; P.split_terms = terms; }
    return launch_mlp(MODE_PLAIN, P, (hipStream_t)stream);
}

PRCNN_API int prcnn_mlp_rows_addinterp(const float* in, int ld_in, int K, const float* wpack, const float* bias, int Nout,
                                       int relu, const float* y_cl, int ld_y, const int32_t* idx3, const float* w3, int B,
                                       int n, int m, float* out, int ld_out, int col_off, prcnn_stream_t stream) {
    return mlp_rows_addinterp_body("prcnn_mlp_rows_addinterp", false, in, ld_in, K, wpack, nullptr, 0, bias, Nout, relu, y_cl, ld_y, idx3, w3, B, n, m,
                                   out, ld_out, col_off, stream);
}

PRCNN_API int prcnn_mlp_rows_addinterp_split(const float* in, int ld_in, int K, const float* wpack, const void* wsplit, int terms,
                                             const float* bias, int Nout, int relu, const float* y_cl, int ld_y, const int32_t* idx3,
                                             const float* w3, int B, int n, int m, float* out, int ld_out, int col_off,
                                             prcnn_stream_t stream) {
    return mlp_rows_addinterp_body("prcnn_mlp_rows_addinterp_split", true, in, ld_in, K, wpack, wsplit, terms, bias, Nout, relu, y_cl, ld_y, idx3, w3,
                                   B, n, m, out, ld_out, col_off, stream);
}

// prcnn_mlp_group_split: the hoisted form on the split-bf16 layer kernel (wsplit = prcnn_pack_weight_split image of the layer, terms 3 / 6;
// wpack: the fp32 image, read only by rows that hold inf / NaN).  C a multiple of 32, 16-byte aligned feature rows; otherwise, or with
// PRCNN_GROUP_SPLIT=0, the call runs the fp32 layer kernel exactly as prcnn_mlp_group does.
static int mlp_group_body(const char* who, bool split, const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl, int ld_feat,
                          int B, int N, int M, int nsample, int C, const float* act_wx, const float* act_bias, const float* wpack,
                          const void* wsplit, int terms, const float* bias, int Nout, int relu, float* out, int ld_out, int col_off, int pool_ns,
                          const int32_t* groups_dev, prcnn_stream_t stream) {
    PRCNN_REQUIRE(xyz && idx && (!split || wsplit), "%s: null pointer", who);
    if (split) PRCNN_REQUIRE(C > 0 && feat_cl, "%s: the hoisted form needs features (C=%d)", who, C);
    else PRCNN_REQUIRE(C == 0 || feat_cl, "%s: C=%d but feat_cl is null", who, C);
    PRCNN_REQUIRE(B >= 0 && N > 0 && M > 0 && nsample > 0 && C >= 0 && (C == 0 || ld_feat >= C),
                  "%s: bad shape B=%d N=%d M=%d ns=%d C=%d ld=%d", who, B, N, M, nsample, C, ld_feat);
    if (split) PRCNN_REQUIRE(terms == 3 || terms == 6, "%s: terms=%d (3 or 6)", who, terms);
    PRCNN_REQUIRE(ld_out >= col_off + Nout, "%s: ld_out=%d < col_off+Nout", who, ld_out);
    MlpParams P = {};
    fill_out(P, wpack, bias, Nout, relu, out, ld_out, col_off, pool_ns);
    const int rc = fill_group(P, xyz, new_xyz, idx, feat_cl, ld_feat, B, N, M, nsample, C, act_wx, act_bias, groups_dev);
    if (rc) return rc;
    if (split) { P.wsplit = wsplit; P.split_terms = terms; }
    return launch_mlp(MODE_GROUP, P, (hipStream_t)stream);
}

PRCNN_API int prcnn_mlp_group(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl,
                              int ld_feat, int B, int N, int M, int nsample, int C, const float* act_wx,
                              const float* act_bias, const float* wpack, const float* bias, int Nout, int relu,
                              float* out, int ld_out, int col_off, int pool_ns, const int32_t* groups_dev, prcnn_stream_t stream) {
    return mlp_group_body("prcnn_mlp_group", false, xyz, new_xyz, idx, feat_cl, ld_feat, B, N, M, nsample, C, act_wx, act_bias, wpack, nullptr, 0, bias,
                          Nout, relu, out, ld_out, col_off, pool_ns, groups_dev, stream);
}

PRCNN_API int prcnn_mlp_group_split(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl,
                                    int ld_feat, int B, int N, int M, int nsample, int C, const float* act_wx,
                                    const float* act_bias, const float* wpack, const void* wsplit, int terms, const float* bias, int Nout,
                                    int relu, float* out, int ld_out, int col_off, int pool_ns, const int32_t* groups_dev,
                                    prcnn_stream_t stream) {
    return mlp_group_body("prcnn_mlp_group_split", true, xyz, new_xyz, idx, feat_cl, ld_feat, B, N, M, nsample, C, act_wx, act_bias, wpack, wsplit, terms,
                          bias, Nout, relu, out, ld_out, col_off, pool_ns, groups_dev, stream);
}

PRCNN_API int prcnn_mlp_interp(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3,
                               const float* skip_cl, int ld_skip, int B, int n, int m, int C2, int C1,
                               const float* act_bias, const float* wpack, const float* bias, int Nout, int relu,
                               float* out, int ld_out, int col_off, prcnn_stream_t stream) {
    PRCNN_REQUIRE(known_cl && idx3 && w3, "prcnn_mlp_interp: null pointer");
    PRCNN_REQUIRE(C1 == 0 || skip_cl, "prcnn_mlp_interp: C1=%d but skip_cl is null", C1);
    PRCNN_REQUIRE(B >= 0 && n > 0 && m > 0 && C2 > 0 && C1 >= 0 && ld_known >= C2 && (C1 == 0 || ld_skip >= C1),
                  "prcnn_mlp_interp: bad shape B=%d n=%d m=%d C2=%d C1=%d", B, n, m, C2, C1);
    PRCNN_REQUIRE(ld_out >= col_off + Nout, "prcnn_mlp_interp: ld_out=%d < col_off+Nout", ld_out);
    MlpParams P = {};
    fill_out(P, wpack, bias, Nout, relu, out, ld_out, col_off, 0);
    const int rc = fill_interp(P, known_cl, ld_known, idx3, w3, skip_cl, ld_skip, B, n, m, C2, C1, act_bias, false);
    if (rc) return rc;
    return launch_mlp(MODE_INTERP, P, (hipStream_t)stream);
}

PRCNN_API int prcnn_mlp_chain_supported(int mode, int nlayers, const int* nout, int pool_ns) {
    if (!nout || nlayers < 1 || nlayers > 3) return 0;
    if (!(pool_ns == 0 || pool_ns == 16 || pool_ns == 32)) return 0;
    // two wide layers on an un-pooled grouped list: the stack kernel (hoisted form, nsample 1 -- checked again at dispatch)
    if (mode == MODE_GROUP && nlayers == 2 && pool_ns == 0 && nout[0] > 0 && nout[1] > 0 && (nout[0] > 128 || nout[1] > 128) &&
        nb32(nout[0]) <= ST_MAX_NB0 && nb32(nout[1]) <= 16 && !sw_present(SW_NO_STACK))
        return 1;
    for (int l = 0; l < nlayers; l++)
        if (nout[l] <= 0 || nout[l] > 128) return 0;
    return chain_instance_exists(mode, nb32(nout[0]), nlayers > 1 ? nb32(nout[1]) : 0, nlayers > 2 ? nb32(nout[2]) : 0) ? 1 : 0;
}

PRCNN_API int prcnn_mlp_chain_rows(const float* in, int ld_in, int64_t rows, int K, int nlayers,
                                   const float* const* wpack, const float* const* bias, const int* nout,
                                   const int* relu, float* out, int ld_out, int col_off, int pool_ns,
                                   const int32_t* seg_cnt, int seg_rows, prcnn_stream_t stream) {
    PRCNN_REQUIRE(in && ld_in >= K && K > 0 && rows >= 0, "prcnn_mlp_chain_rows: bad input");
    PRCNN_REQUIRE(!seg_cnt || (seg_rows > 0 && seg_rows % 128 == 0 && rows % seg_rows == 0 && pool_ns == 0),
                  "prcnn_mlp_chain_rows: seg_rows=%d must be a multiple of 128 dividing rows (and no pooling)", seg_rows);
    ChainParams C = {};
    int rc = fill_chain(C, nlayers, wpack, bias, nout, relu, out, ld_out, col_off, pool_ns);
    if (rc) return rc;
    PRCNN_REQUIRE(pool_ns == 0 || rows % pool_ns == 0, "prcnn_mlp_chain_rows: rows not a multiple of pool_ns");
    fill_plain(C.a, in, ld_in, rows, K);
    C.a.seg_cnt = seg_cnt; C.a.seg_rows = seg_rows;
    return dispatch_chain(MODE_PLAIN, C, (hipStream_t)stream);
}

// the checks and fills of prcnn_mlp_chain_group (prcnn_mlp_chain_group_multi runs them per problem, under the same messages)
static int fill_chain_group(ChainParams& C, const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl, int ld_feat, int B, int N,
                            int M, int nsample, int C_, const float* act_wx, const float* act_bias, int nlayers, const float* const* wpack,
                            const float* const* bias, const int* nout, const int* relu, float* out, int ld_out, int col_off, int pool_ns,
                            const int32_t* groups_dev) {
    PRCNN_REQUIRE(xyz && idx && (C_ == 0 || feat_cl), "prcnn_mlp_chain_group: null pointer");
    PRCNN_REQUIRE(B >= 0 && N > 0 && M > 0 && nsample > 0 && C_ >= 0 && (C_ == 0 || ld_feat >= C_), "prcnn_mlp_chain_group: bad shape");
    int rc = fill_chain(C, nlayers, wpack, bias, nout, relu, out, ld_out, col_off, pool_ns);
    if (rc) return rc;
    PRCNN_REQUIRE(pool_ns == 0 || pool_ns == nsample, "prcnn_mlp_chain_group: pool_ns must equal nsample");
    return fill_group(C.a, xyz, new_xyz, idx, feat_cl, ld_feat, B, N, M, nsample, C_, act_wx, act_bias, groups_dev);
}

PRCNN_API int prcnn_mlp_chain_group(const float* xyz, const float* new_xyz, const int32_t* idx, const float* feat_cl,
                                    int ld_feat, int B, int N, int M, int nsample, int C_, const float* act_wx,
                                    const float* act_bias, int nlayers,
                                    const float* const* wpack, const float* const* bias, const int* nout,
                                    const int* relu, float* out, int ld_out, int col_off, int pool_ns,
                                    const int32_t* groups_dev, prcnn_stream_t stream) {
    ChainParams C = {};
    const int rc = fill_chain_group(C, xyz, new_xyz, idx, feat_cl, ld_feat, B, N, M, nsample, C_, act_wx, act_bias, nlayers, wpack, bias, nout, relu, out,
                                    ld_out, col_off, pool_ns, groups_dev);
    if (rc) return rc;
    return dispatch_chain(MODE_GROUP, C, (hipStream_t)stream);
}

PRCNN_API int prcnn_mlp_chain_interp(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3,
                                     const float* skip_cl, int ld_skip, int B, int n, int m, int C2, int C1,
                                     const float* act_bias, int nlayers, const float* const* wpack, const float* const* bias,
                                     const int* nout, const int* relu, float* out, int ld_out, int col_off,
                                     prcnn_stream_t stream) {
    PRCNN_REQUIRE(known_cl && idx3 && w3 && (C1 == 0 || skip_cl), "prcnn_mlp_chain_interp: null pointer");
    PRCNN_REQUIRE(B >= 0 && n > 0 && m > 0 && C2 > 0 && C1 >= 0 && ld_known >= C2 && (C1 == 0 || ld_skip >= C1), "prcnn_mlp_chain_interp: bad shape");
    ChainParams C = {};
    int rc = fill_chain(C, nlayers, wpack, bias, nout, relu, out, ld_out, col_off, 0);
    if (rc) return rc;
    rc = fill_interp(C.a, known_cl, ld_known, idx3, w3, skip_cl, ld_skip, B, n, m, C2, C1, act_bias, true);
    if (rc) return rc;
    return dispatch_chain(MODE_INTERP, C, (hipStream_t)stream);
}

// Two-layer plain-row chain on the split kernels; shapes: K = 128, nout[0] = 128, nout[1] = 1 or 65..128 (the RPN heads).
// wchain[l]: prcnn_pack_weight_split(chain = 1) images; wpack1: the fp32 pack image of layer 1 (read by the single-channel output).
// PRCNN_EUNSUPPORTED for any other shape: the caller issues prcnn_mlp_chain_rows.
PRCNN_API int prcnn_mlp_chain_rows_split(const float* in, int ld_in, int64_t rows, int K, const void* const* wchain, const float* const* wpack,
                                         const float* const* bias, const int* nout, const int* relu, int terms, float* out, int ld_out,
                                         int col_off, prcnn_stream_t stream) {
    PRCNN_REQUIRE(in && wchain && wpack && bias && nout && relu && out, "prcnn_mlp_chain_rows_split: null pointer");
    PRCNN_REQUIRE(terms == 3 || terms == 6, "prcnn_mlp_chain_rows_split: terms=%d (3 or 6)", terms);
    PRCNN_REQUIRE(wpack[0] && wpack[1] && aligned16(wpack[0]) && aligned16(wpack[1]), "prcnn_mlp_chain_rows_split: the fp32 pack images of both layers are needed (non-finite rows, single-channel output)");
    const bool ok = K == 128 && nout[0] == 128 && (nout[1] == 1 || (nout[1] > 64 && nout[1] <= 128)) && aligned16(in) && ld_in % 4 == 0 &&
                    ld_in >= K && wchain[0] && (nout[1] == 1 || wchain[1] != nullptr);
    if (!ok) return PRCNN_EUNSUPPORTED;
    PRCNN_REQUIRE(ld_out >= col_off + nout[1], "prcnn_mlp_chain_rows_split: ld_out=%d < col_off+Nout", ld_out);
    if (rows == 0) return PRCNN_OK;
    ChainParams C = {};
    MlpParams& P = C.a;
    fill_out(P, wpack[0], bias[0], nout[0], relu[0], out, ld_out, col_off, 0);
    P.rows = rows; P.K = K; P.in = in; P.ld_in = ld_in; P.rows_unit = 1;      // (not fill_plain: this export has always left vec_a 0)
    P.wsplit = wchain[0]; P.split_terms = terms;
    C.wsplit1 = wchain[1]; C.wpack1 = wpack[1]; C.bias1 = bias[1]; C.N1 = nout[1]; C.relu1 = relu[1]; C.KB1 = 16; C.nlayers = 2;
    MlpLaunch L;
    decide_chain_split(MODE_PLAIN, nout[1] == 1 ? 1 : nout[1] <= 96 ? 3 : 4, terms, (long)rows * ld_in < (1L << 30), rows,
                       "prcnn_mlp_chain_rows_split", L);
    return mlp_launch(L, P, &C, (hipStream_t)stream);
}

// Hoisted FP0 on the split chain kernel: rows relu(interp(known_cl) + act_bias) (C2 = 128, no skip features) through ONE
// 128 -> 128 layer.  wchain: prcnn_pack_weight_split(chain = 1).  PRCNN_EUNSUPPORTED for other shapes (issue prcnn_mlp_chain_interp).
PRCNN_API int prcnn_mlp_chain_interp_split(const float* known_cl, int ld_known, const int32_t* idx3, const float* w3, int B, int n,
                                           int m, int C2, const float* act_bias, const void* wchain, const float* wpack, const float* bias,
                                           int Nout, int relu, int terms, float* out, int ld_out, int col_off, prcnn_stream_t stream) {
    PRCNN_REQUIRE(known_cl && idx3 && w3 && act_bias && wchain && wpack && aligned16(wpack) && out, "prcnn_mlp_chain_interp_split: null / misaligned pointer");
    PRCNN_REQUIRE(terms == 3 || terms == 6, "prcnn_mlp_chain_interp_split: terms=%d (3 or 6)", terms);
    PRCNN_REQUIRE(B >= 0 && n > 0 && m > 0 && ld_known >= C2 && ld_out >= col_off + Nout, "prcnn_mlp_chain_interp_split: bad shape");
    if (!(C2 == 128 && Nout == 128 && aligned16(known_cl) && ld_known % 4 == 0 && aligned16(act_bias))) return PRCNN_EUNSUPPORTED;
    if (B == 0) return PRCNN_OK;
    ChainParams C = {};
    MlpParams& P = C.a;
    fill_out(P, wpack, bias, Nout, relu, out, ld_out, col_off, 0);
    const int rc = fill_interp(P, known_cl, ld_known, idx3, w3, nullptr, 0, B, n, m, C2, 0, act_bias, true);      // (cannot fail: checked above)
    if (rc) return rc;
    P.rows_unit = 1;
    P.wsplit = wchain; P.split_terms = terms;
    C.nlayers = 1;
    MlpLaunch L;
    decide_chain_split(MODE_INTERP, 0, terms, (long)B * m * ld_known < (1L << 30), P.rows, "prcnn_mlp_chain_interp_split", L);
    return mlp_launch(L, P, &C, (hipStream_t)stream);
}
