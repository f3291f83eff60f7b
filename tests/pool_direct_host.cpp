// Stand-alone host program (tests/test_pool_direct_cpu.py; built like tests/mlp_launch_record.cpp, once plain and once with
// -fsanitize=address,undefined): what prcnn_mlp_chain_group_multi_dst launches next to prcnn_mlp_chain_group_multi, recorded and not
// launched, for the four set-abstraction levels of the RPN --
//   * without destination lists the new export records what the old one records: kernel instance, grid, block, dynamic LDS and every
//     problem's parameters, the store-by-destination fields zero;
//   * with them, kernel instance, grid, block and LDS stay what they were and every problem carries its list in the right field
//     (row_dst for an un-pooled problem, grp_dst for a pooled one) with the shared output and its own column offset
// -- and a plain C++ twin of the split's destination rule (dedup.hip, group_compact_body) on hand-made index rows.
#include "launch_record_prelude.h"

struct MultiParams;
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const MultiParams& M);

#include "mlp.hip"

static unsigned long pv(const void* p) { return (unsigned long)reinterpret_cast<uintptr_t>(p); }
static void rec_params(const MlpParams& P) {
    recf(" P{rows %ld K %d Nout %d out %lx ld_out %d col_off %d pool_ns %d idx %lx feat %lx N %d M %d ns %d C %d act %d rows_dev %lx unit %d", P.rows, P.K, P.Nout,
         pv(P.out), P.ld_out, P.col_off, P.pool_ns, pv(P.idx), pv(P.feat), P.N, P.M, P.ns, P.C, P.act, pv(P.rows_dev), P.rows_unit);
    recf(" row_dst %lx grp_dst %lx out2 %lx ld_out2 %d col_off2 %d}", pv(P.row_dst), pv(P.grp_dst), pv(P.out2), P.ld_out2, P.col_off2);
}
static void rec_params(const ChainParams& C) {
    rec_params(C.a);
    recf(" C{N1 %d N2 %d nlayers %d stack_split %d}", C.N1, C.N2, C.nlayers, C.stack_split);
}
static MultiParams g_last;
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const MultiParams& M) {
    rec_head(k, g, b, lds);
    g_last = M;
    for (int p = 0; p < M.U.nprob; p++) {
        recf(" [%d v%d]", p, M.variant[p]);
        rec_params(M.c[p]);
    }
}

template <class T = float> static T* A(int i) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (i + 1)); }

static int g_bad = 0;
#define CHECK(c, ...)                                     \
    do {                                                  \
        if (!(c)) {                                       \
            g_bad++;                                      \
            printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            printf(__VA_ARGS__);                          \
            printf("\n");                                 \
        }                                                 \
    } while (0)

struct Stack {
    int nlayers;
    const float* wpack[3];
    const float* bias[3];
    int nout[3], relu[3];
    Stack(std::initializer_list<int> widths) : nlayers((int)widths.size()) {
        int l = 0;
        for (int w : widths) { wpack[l] = A(20 + l); bias[l] = A(24 + l); nout[l] = w; relu[l] = 1; l++; }
    }
};

// the flat list (un-pooled, nsample 1, G * T rows) or the dense list (pooled, G groups of ns rows) of one scale
static prcnn_chain_group_problem_t problem(const Stack& s, int C, int G, int T, int ns, bool dense, float* out, int ld_out, int col_off, int slot) {
    prcnn_chain_group_problem_t p = {};
    p.xyz = A(0); p.new_xyz = A(1 + slot); p.idx = A<const int32_t>(5 + slot);
    p.feat_cl = C ? A(9) : nullptr; p.act_wx = C ? A(10) : nullptr; p.act_bias = C ? A(11) : nullptr;
    p.wpack = s.wpack; p.bias = s.bias; p.nout = s.nout; p.relu = s.relu;
    p.out = out; p.groups_dev = A<const int32_t>(12 + slot);
    p.ld_feat = C; p.B = 1; p.N = 4 * 16384; p.M = dense ? G : G * T; p.nsample = dense ? ns : 1; p.C = C; p.nlayers = s.nlayers;
    p.ld_out = ld_out; p.col_off = col_off; p.pool_ns = dense ? ns : 0;
    return p;
}

static std::string head_of(const std::string& rec) { return rec.substr(0, rec.find(" [0 ")); }

static void level(const char* name, const char* kernel, const Stack& a, int ns_a, const Stack& b, int ns_b, int C, int G, bool all_flat) {
    const int ca = a.nout[a.nlayers - 1], cb = b.nout[b.nlayers - 1], ld2 = ca + cb;
    float* out2 = A(40);
    prcnn_chain_group_problem_t old_p[4], new_p[4];
    const int32_t* dst[4] = {nullptr, nullptr, nullptr, nullptr};
    int col2[4] = {0, 0, 0, 0};
    int n = 0;
    // heaviest first, as pointnet2_modules._forward_merged orders them: flat b, flat a, then the dense lists
    const int Ta = all_flat ? ns_a : ns_a / 4, Tb = all_flat ? ns_b : ns_b / 4;
    old_p[n] = new_p[n] = problem(b, C, G, Tb, ns_b, false, A(30), cb, 0, 0); dst[n] = A<const int32_t>(50); col2[n] = ca; n++;
    old_p[n] = new_p[n] = problem(a, C, G, Ta, ns_a, false, A(31), ca, 0, 1); dst[n] = A<const int32_t>(51); col2[n] = 0; n++;
    if (!all_flat) {
        old_p[n] = problem(b, C, G, Tb, ns_b, true, A(32), cb, 0, 2);
        new_p[n] = problem(b, C, G, Tb, ns_b, true, out2, ld2, ca, 2); dst[n] = A<const int32_t>(52); col2[n] = ca; n++;
        old_p[n] = problem(a, C, G, Ta, ns_a, true, A(33), ca, 0, 3);
        new_p[n] = problem(a, C, G, Ta, ns_a, true, out2, ld2, 0, 3); dst[n] = A<const int32_t>(53); col2[n] = 0; n++;
    }
    auto run = [&](int which, std::string& rec) {
        g_rec.clear();
        g_launches = 0;
        const int rc = which == 0   ? prcnn_mlp_chain_group_multi(n, old_p, nullptr)
                       : which == 1 ? prcnn_mlp_chain_group_multi_dst(n, old_p, nullptr, nullptr, 0, nullptr, nullptr)
                                    : prcnn_mlp_chain_group_multi_dst(n, new_p, dst, out2, ld2, col2, nullptr);
        CHECK(rc == 0 && g_launches == 1, "%s: call %d gave rc %d and %d launches:%s", name, which, rc, g_launches, g_rec.c_str());
        rec = g_rec;
    };
    std::string r_old, r_null, r_dst;
    run(0, r_old);
    run(1, r_null);
    CHECK(r_old == r_null, "%s: without destination lists the new export records\n%s\nthe old one\n%s", name, r_null.c_str(), r_old.c_str());
    CHECK(r_old.find(kernel) != std::string::npos, "%s: expected an instance of %s, got%s", name, kernel, head_of(r_old).c_str());
    CHECK(r_old.find("row_dst 0 grp_dst 0 out2 0 ld_out2 0 col_off2 0") != std::string::npos, "%s: the old export leaves the new fields zero", name);
    run(2, r_dst);
    CHECK(head_of(r_dst) == head_of(r_old), "%s: with destination lists the launch is\n%s\nnot\n%s", name, head_of(r_dst).c_str(), head_of(r_old).c_str());
    CHECK(g_last.U.nprob == n, "%s: %d problems launched, %d given", name, g_last.U.nprob, n);
    for (int p = 0; p < n && p < g_last.U.nprob; p++) {
        const MlpParams& P = g_last.c[p].a;
        const bool pooled = P.pool_ns != 0;
        CHECK((pooled ? P.grp_dst : P.row_dst) == dst[p] && (pooled ? P.row_dst : P.grp_dst) == nullptr, "%s: problem %d carries its list in the wrong field", name, p);
        CHECK(P.out2 == out2 && P.ld_out2 == ld2 && P.col_off2 == col2[p], "%s: problem %d: out2 %lx ld %d col %d", name, p, pv(P.out2), P.ld_out2, P.col_off2);
        CHECK(pooled == (p >= 2), "%s: problem %d pooled %d", name, p, (int)pooled);
    }
    printf("%s:%s\n", name, head_of(r_dst).c_str());
}

// ---- the split's destination rule (dedup.hip, group_compact_body): a group's real rows are its leading distinct indices -- the
// padding repeats idx[0]; a sparse group (cnt <= T) with ONE real row names its own output row, the rows of any other stay (-1)
static int rdst_rule(const int32_t* row, int ns, int T, int g, int32_t* rdst) {
    int cnt = ns;
    for (int s = 1; s < ns; s++)
        if (row[s] == row[0]) { cnt = s; break; }
    if (cnt > T) return 0;                                   // dense: no flat rows
    for (int s = 0; s < cnt; s++) rdst[s] = cnt == 1 ? g : -1;
    return cnt;
}

static void rdst_cases() {
    struct Case { std::vector<int32_t> row; int T, g, rows; std::vector<int32_t> want; };
    const Case cases[] = {
        {{7, 7, 7, 7, 7, 7, 7, 7}, 2, 5, 1, {5}},            // only the centroid: the first index repeats at position 1
        {{7, 7, 9, 11, 7, 7, 7, 7}, 2, 6, 1, {6}},           // a repeat at position 1 ends the real rows whatever follows
        {{3, 8, 3, 3, 3, 3, 3, 3}, 2, 0, 2, {-1, -1}},       // two real rows: pooled
        {{3, 8, 9, 3, 3, 3, 3, 3}, 4, 9, 3, {-1, -1, -1}},
        {{3, 8, 9, 3, 3, 3, 3, 3}, 2, 9, 0, {}},             // more than T: the dense list
        {{0, 1, 2, 3, 4, 5, 6, 7}, 8, 2, 8, {-1, -1, -1, -1, -1, -1, -1, -1}},      // a full group on an all-flat scale
        {{0, 1, 2, 3, 4, 5, 6, 7}, 2, 2, 0, {}},
        {{4}, 1, 3, 1, {3}},                                  // nsample 1
        {{0, 0, 0, 0}, 1, 0, 1, {0}},                         // group 0 is a destination, not "stays" (>= 0)
    };
    for (const Case& c : cases) {
        std::vector<int32_t> got(c.row.size(), -7);
        const int rows = rdst_rule(c.row.data(), (int)c.row.size(), c.T, c.g, got.data());
        CHECK(rows == c.rows, "rdst rule: %d rows, expected %d", rows, c.rows);
        for (int s = 0; s < (int)got.size(); s++)
            CHECK(got[s] == (s < (int)c.want.size() ? c.want[s] : -7), "rdst rule: row %d of group %d is %d", s, c.g, got[s]);
    }
}

int main() {
    // SA1: xyz only, three narrow layers, sparse lists of ns / 4 rows next to dense lists
    level("SA1", "sa0_multi_kernel", Stack{16, 16, 32}, 16, Stack{32, 32, 64}, 32, 0, 4 * 4096, false);
    // SA2: hoisted first layer (Z of 64 channels), 64 -> 64 | 96 -> 128
    level("SA2", "chain_fast_multi_kernel", Stack{64, 128}, 16, Stack{96, 128}, 32, 64, 4 * 1024, false);
    // SA3 / SA4: the two-layer stacks on all-flat lists
    level("SA3", "stack2_multi_kernel", Stack{196, 256}, 16, Stack{196, 256}, 32, 128, 4 * 256, true);
    level("SA4", "stack2_multi_kernel", Stack{256, 512}, 16, Stack{384, 512}, 32, 256, 4 * 64, true);
    rdst_cases();
    printf("%d failed\n", g_bad);
    return g_bad ? 1 : 0;
}
