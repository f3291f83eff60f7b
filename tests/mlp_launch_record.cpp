// Stand-alone host program: which kernel instance, grid, block, dynamic LDS and params every MLP export of csrc/mlp.hip launches,
// over a sweep of arguments and switches -- recorded, not launched.  Compiled as HIP host code only (hipcc -x hip --cuda-host-only);
// no device is touched: the launch macro records, the device queries answer "device 0, 256 CUs", the LDS-limit raise succeeds.
// MLP_SOURCE names the unit to include (default: the tree's mlp.hip), so the same program built against an older mlp.hip gives the
// records to compare with: tests/golden/mlp_launch_digests.txt holds those of the last commit whose launches were checked on
// a device.  A kernel is named by its instantiation (template arguments resolved), not by the text of the launch expression.
// Built and run by tests/test_mlp_host_cpu.py (once plain, once with -fsanitize=address,undefined).
//   mlp_launch_record            per (switch setting, export): number of calls and an FNV-1a digest of their records
//   mlp_launch_record --dump     every record
#include "launch_record_prelude.h"

#ifndef MLP_SOURCE
#define MLP_SOURCE "mlp.hip"
#endif
#include MLP_SOURCE

static unsigned long pv(const void* p) { return (unsigned long)reinterpret_cast<uintptr_t>(p); }
static void rec_params(const MlpParams& P) {
    recf(" P{rows %ld K %d KB %d NB %d wpack %lx bias %lx Nout %d relu %d out %lx ld_out %d col_off %d pool_ns %d in %lx ld_in %d", P.rows, P.K, P.KB, P.NB,
         pv(P.wpack), pv(P.bias), P.Nout, P.relu, pv(P.out), P.ld_out, P.col_off, P.pool_ns, pv(P.in), P.ld_in);
    recf(" xyz %lx new_xyz %lx idx %lx feat %lx ld_feat %d N %d M %d ns %d C %d", pv(P.xyz), pv(P.new_xyz), pv(P.idx), pv(P.feat), P.ld_feat, P.N, P.M, P.ns, P.C);
    recf(" known %lx idx3 %lx w3 %lx skip %lx ld_known %d ld_skip %d n %d m %d C2 %d C1 %d vec %d,%d", pv(P.known), pv(P.idx3), pv(P.w3), pv(P.skip), P.ld_known,
         P.ld_skip, P.n, P.m, P.C2, P.C1, P.vec_a, P.vec_b);
    recf(" act %d wx %lx ab %lx addY %lx ldY %d rows_dev %lx unit %d seg %lx,%d xcd_tpf %d wgm_cols %d addy_phase %d wsplit %lx terms %d}", P.act, pv(P.act_wx),
         pv(P.act_bias), pv(P.addY), P.ldY, pv(P.rows_dev), P.rows_unit, pv(P.seg_cnt), P.seg_rows, P.xcd_tpf, P.wgm_cols, P.addy_phase, pv(P.wsplit), P.split_terms);
}
static void rec_params(const ChainParams& C) {
    rec_params(C.a);
    recf(" C{w1 %lx b1 %lx KB1 %d N1 %d relu1 %d w2 %lx b2 %lx KB2 %d N2 %d relu2 %d nlayers %d stack_split %d wsplit1 %lx}", pv(C.wpack1), pv(C.bias1), C.KB1, C.N1,
         C.relu1, pv(C.wpack2), pv(C.bias2), C.KB2, C.N2, C.relu2, C.nlayers, C.stack_split, pv(C.wsplit1));
}

// ---- the sweep ------------------------------------------------------------------------------------------------------------
// dummy pointers: never dereferenced.  A(i): 16-byte aligned; U(i): 4-byte aligned only
template <class T = float> static T* A(int i) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (i + 1)); }
template <class T = float> static T* U(int i) { return reinterpret_cast<T*>((uintptr_t)0x10000 * (i + 1) + 4); }
static const int32_t* AI(int i) { return A<const int32_t>(i); }

struct Group { std::string name; long calls = 0; unsigned long long h = 1469598103934665603ull; };
static std::vector<Group> g_groups;
static bool g_dump = false;
static std::string g_setting;
static int g_inconsistent = 0;

// ends a call: files its record under (setting, export); returns whether the call launched anything
static bool done(const char* exp, int rc) {
    const std::string key = g_setting + " " + exp;
    size_t gi = 0;
    while (gi < g_groups.size() && g_groups[gi].name != key) gi++;
    if (gi == g_groups.size()) g_groups.push_back({key});
    Group& g = g_groups[gi];
    char head[64];
    snprintf(head, sizeof head, "#%ld rc %d", g.calls, rc);
    const std::string line = head + g_rec;
    for (unsigned char ch : line) g.h = (g.h ^ ch) * 1099511628211ull;
    g.h = (g.h ^ '\n') * 1099511628211ull;
    g.calls++;
    if (g_dump) printf("%s %s\n", key.c_str(), line.c_str());
    const bool launched = g_launches > 0;
    g_rec.clear();
    g_launches = 0;
    return launched;
}

static const long ROWS[] = {0, 1, 127, 128, 129, 4096, 4097};
static const int KS[] = {3, 8, 32, 96, 128, 256, 264, 512, R32_MAX_K - 8, R32_MAX_K, R32_MAX_K + 8};
static const int NOUTS[] = {1, 16, 64, 65, 96, 97, 128, 129, 512};
static const int POOLS[] = {0, 16, 32, 64};

static void sweep_rows() {
    for (int split = 0; split < 2; split++)
        for (int terms : {3, 6}) {
            if (!split && terms == 6) continue;
            const char* exp = split ? "prcnn_mlp_rows_split" : "prcnn_mlp_rows";
            auto call = [&](const float* in, int ld_in, long rows, int K, int Nout, int pool, const int32_t* rows_dev, int unit, const int32_t* seg, int seg_rows) {
                const int rc = split ? prcnn_mlp_rows_split(in, ld_in, rows, K, A(1), A<void>(2), terms, A(3), Nout, 1, A(4), Nout + 8, 8, pool, rows_dev, unit, seg,
                                                            seg_rows, nullptr)
                                     : prcnn_mlp_rows(in, ld_in, rows, K, A(1), A(3), Nout, 1, A(4), Nout + 8, 8, pool, rows_dev, unit, seg, seg_rows, nullptr);
                done(exp, rc);
            };
            for (long rows : ROWS)
                for (int K : KS)
                    for (int Nout : NOUTS)
                        for (int pool : POOLS) {
                            call(A(0), K + (4 - K % 4) % 4, rows, K, Nout, pool, nullptr, 1, nullptr, 0);
                            if (pool == 0 && Nout % 32 == 0) {
                                call(U(0), K + (4 - K % 4) % 4, rows, K, Nout, pool, nullptr, 1, nullptr, 0);          // vec_a off
                                call(A(0), K + 1, rows, K, Nout, pool, AI(5), 0, nullptr, 0);                          // device-side row count
                                call(A(0), K + (4 - K % 4) % 4, rows, K, Nout, pool, nullptr, 1, AI(6), 128);         // live-row segments
                                call(A(0), K + (4 - K % 4) % 4, rows, K, Nout, pool, AI(5), 4, nullptr, 0);
                            }
                        }
            // few columns on very many rows (the bounded narrow grid), and wide tiles on rows that cannot take vector loads
            for (long rows : {2048L * 128, 2049L * 128, 4100L * 128}) {
                call(A(0), 32, rows, 32, 64, 0, AI(5), 1, nullptr, 0);
                call(U(0), 128, rows, 128, 512, 0, nullptr, 1, nullptr, 0);
            }
            // tile counts on both sides of 192, 384, 1024 and 2048: wide tiles = row tiles * ceil(NB / 4), narrow = row tiles * ceil(NB / 2)
            for (int Nout : {128, 256, 512})
                for (int K : {128, 512})
                    for (long wide_tiles : {191L, 192L, 193L, 383L, 384L, 385L, 1023L, 1024L, 1025L, 2047L, 2048L, 2049L, 4100L}) {
                        const long row_tiles = (wide_tiles + Nout / 128 - 1) / (Nout / 128);
                        for (long rows : {row_tiles * 128, row_tiles * 128 - 127, (row_tiles - 1) * 128}) {
                            call(A(0), K, rows, K, Nout, 0, nullptr, 1, nullptr, 0);
                            call(A(0), K, rows, K, Nout, 0, AI(5), 1, nullptr, 0);
                            call(A(0), K, rows / 128 * 128, K, Nout, 0, nullptr, 1, AI(6), 128);
                        }
                    }
        }
}

static void sweep_addinterp() {
    for (int split = 0; split < 2; split++)
        for (int terms : {3, 6}) {
            if (!split && terms == 6) continue;
            for (int B : {0, 1, 8, 33})
                for (int n : {1, 127, 128, 4097, 16384})
                    for (int K : {3, 32, 96, 128, 264})
                        for (int Nout : {64, 97, 128, 512})
                            for (int al = 0; al < 2; al++) {
                                const float* in = al ? U(0) : A(0);
                                const int rc = split ? prcnn_mlp_rows_addinterp_split(in, K + (4 - K % 4) % 4, K, A(1), A<void>(2), terms, A(3), Nout, 1, A(4), Nout, AI(5), A(6),
                                                                                      B, n, 64, A(7), Nout, 0, nullptr)
                                                     : prcnn_mlp_rows_addinterp(in, K + (4 - K % 4) % 4, K, A(1), A(3), Nout, 1, A(4), Nout, AI(5), A(6), B, n, 64, A(7), Nout,
                                                                                0, nullptr);
                                done(split ? "prcnn_mlp_rows_addinterp_split" : "prcnn_mlp_rows_addinterp", rc);
                            }
        }
}

static void sweep_group() {
    for (int split = 0; split < 2; split++)
        for (int terms : {3, 6}) {
            if (!split && terms == 6) continue;
            for (int B : {0, 1, 16})
                for (int M : {1, 129, 4096})
                    for (int ns : {1, 16, 32, 64})
                        for (int C : {0, 8, 32, 96, 128, 264})
                            for (int Nout : {16, 64, 97, 128, 512})
                                for (int form = 0; form < 4; form++) {          // 0 plain gather, 1 hoisted, 2 hoisted + row count, 3 unaligned features
                                    if (split && C == 0) continue;
                                    const float* feat = C == 0 ? nullptr : form == 3 ? U(3) : A(3);
                                    const float* wx = form == 1 || form == 2 ? A(4) : nullptr;
                                    const float* ab = form == 1 || form == 2 ? A(5) : nullptr;
                                    const int32_t* gd = form == 2 ? AI(6) : nullptr;
                                    for (int pool : {0, ns}) {
                                        const int rc = split ? prcnn_mlp_group_split(A(0), A(1), AI(2), feat, C, B, 16384, M, ns, C, wx, ab, A(7), A<void>(8), terms, A(9), Nout,
                                                                                     1, A(10), Nout, 0, pool, gd, nullptr)
                                                             : prcnn_mlp_group(A(0), A(1), AI(2), feat, C, B, 16384, M, ns, C, wx, ab, A(7), A(9), Nout, 1, A(10), Nout, 0, pool,
                                                                               gd, nullptr);
                                        done(split ? "prcnn_mlp_group_split" : "prcnn_mlp_group", rc);
                                    }
                                }
        }
}

static void sweep_interp() {
    for (int B : {0, 1, 8, 16})
        for (int n : {1, 128, 129, 4096, 16384})
            for (int C2 : {8, 32, 128, 256, 262})
                for (int C1 : {0, 3, 32, 128})
                    for (int Nout : {64, 97, 128, 512})
                        for (int form = 0; form < 3; form++) {          // 0 plain, 1 hoisted, 2 unaligned sources
                            const float* known = form == 2 ? U(0) : A(0);
                            const float* skip = C1 == 0 ? nullptr : form == 2 ? U(3) : A(3);
                            const int rc = prcnn_mlp_interp(known, C2 + (4 - C2 % 4) % 4, AI(1), A(2), skip, C1, B, n, 512, C2, C1, form == 1 ? A(4) : nullptr, A(5), A(6),
                                                            Nout, 1, A(7), Nout + 4, 4, nullptr);
                            done("prcnn_mlp_interp", rc);
                        }
}

// nout == 0 ends a stack; every row of the chain table, triples that are not in it, the stack and SA0 shapes
static const int WIDTHS[][3] = {{32, 32, 32}, {32, 32, 64}, {64, 64, 128}, {64, 96, 128}, {64, 128, 0}, {96, 128, 0}, {128, 128, 0}, {128, 0, 0}, {128, 1, 0},
                                {128, 96, 0}, {128, 65, 0}, {16, 16, 32}, {32, 32, 64}, {16, 16, 30}, {64, 64, 64}, {128, 128, 128}, {32, 0, 0}, {96, 96, 0},
                                {196, 256, 0}, {256, 512, 0}, {384, 512, 0}, {128, 129, 0}, {400, 256, 0}, {129, 128, 128}, {512, 0, 0}};
static bool g_check_supported = true;
// rows: whether the call has any (a call without rows succeeds and launches nothing, whatever its widths)
static void chain_done(const char* exp, int mode, int nl, const int* nout, int pool, int rc, bool wide_ok, bool rows) {
    const bool launched = done(exp, rc);
    if (!g_check_supported || !rows || rc == PRCNN_EINVAL) return;
    const bool sup = prcnn_mlp_chain_supported(mode, nl, nout, pool) != 0;
    bool wide = false;
    for (int l = 0; l < nl; l++) wide |= nout[l] > 128;
    // register chains (every width <= 128): offered exactly where dispatch launches.  The stack (a width > 128) is offered for every grouped
    // pair of wide layers and launched for the hoisted nsample-1 form of it (wide_ok): there, offered and launched must agree too.
    const bool bad = wide ? (launched && !sup) || (wide_ok && sup && !launched) : sup != launched;
    if (bad) {
        g_inconsistent++;
        printf("INCONSISTENT %s mode %d widths %d,%d,%d pool %d: supported %d launched %d rc %d\n", exp, mode, nout[0], nl > 1 ? nout[1] : 0, nl > 2 ? nout[2] : 0, pool,
               (int)sup, (int)launched, rc);
    }
}

static void sweep_chains() {
    const float* wp[3] = {A(10), A(11), A(12)};
    const float* bs[3] = {A(13), nullptr, A(14)};
    const int relu[3] = {1, 1, 0};
    for (const int* w : WIDTHS) {
        const int nl = w[1] == 0 ? 1 : w[2] == 0 ? 2 : 3;
        const int last = w[nl - 1];
        for (long rows : {0L, 1L, 128L, 129L, 4097L})
            for (int K : {3, 8, 32, 96, 128, 136, 256})
                for (int form = 0; form < 3; form++)          // 0 aligned, 1 unaligned, 2 live-row segments
                    for (int pool : {0, 16, 32}) {
                        const long r = form == 2 ? rows / 128 * 128 : pool ? rows / pool * pool : rows;
                        const int rc = prcnn_mlp_chain_rows(form == 1 ? U(0) : A(0), K + (4 - K % 4) % 4, r, K, nl, wp, bs, w, relu, A(4), last, 0, form == 2 ? 0 : pool,
                                                            form == 2 ? AI(5) : nullptr, form == 2 ? 128 : 0, nullptr);
                        chain_done("prcnn_mlp_chain_rows", MODE_PLAIN, nl, w, form == 2 ? 0 : pool, rc, false, r > 0);
                    }
        for (int B : {0, 1, 16})
            for (int M : {1, 4096})
                for (int ns : {1, 16, 32})
                    for (int C : {0, 8, 64, 128, 256, 264})
                        for (int form = 0; form < 3; form++) {          // 0 plain gather, 1 hoisted, 2 hoisted on unaligned features
                            if (form && C == 0) continue;
                            for (int pool : {0, ns}) {
                                if (pool == 1) continue;
                                const int rc = prcnn_mlp_chain_group(A(0), (C == 8 && form == 0) ? nullptr : A(1), AI(2), C ? (form == 2 ? U(3) : A(3)) : nullptr, C, B, 16384, M,
                                                                     ns, C, form ? A(5) : nullptr, form ? A(6) : nullptr, nl, wp, bs, w, relu, A(4), last, 0, pool, AI(7), nullptr);
                                chain_done("prcnn_mlp_chain_group", MODE_GROUP, nl, w, pool, rc,
                                           form == 1 && ns == 1 && C % 8 == 0 && C <= ST_MAX_K0 && nl == 2, B > 0);
                            }
                        }
        for (int B : {0, 1, 8})
            for (int n : {1, 128, 4096})
                for (int C2 : {8, 64, 128, 136})
                    for (int C1 : {0, 32})
                        for (int form = 0; form < 3; form++) {          // 0 plain, 1 hoisted, 2 unaligned
                            const int rc = prcnn_mlp_chain_interp(form == 2 ? U(0) : A(0), C2, AI(1), A(2), C1 ? A(3) : nullptr, C1, B, n, 512, C2, C1, form == 1 ? A(5) : nullptr,
                                                                  nl, wp, bs, w, relu, A(4), last, 0, nullptr);
                            chain_done("prcnn_mlp_chain_interp", MODE_INTERP, nl, w, 0, rc, false, B > 0);
                        }
    }
}

static void sweep_split_chains() {
    const void* wc[2] = {A<void>(10), A<void>(11)};
    const float* wp[2] = {A(12), A(13)};
    const float* bs[2] = {A(14), A(15)};
    const int relu[2] = {1, 0};
    for (int terms : {3, 6})
        for (int n1 : {1, 2, 64, 65, 96, 97, 128, 129})
            for (int K : {128, 96})
                for (int al = 0; al < 2; al++)
                    for (long rows : {0L, 1L, 128L, 4097L, (1L << 30) / 128 - 1, (1L << 30) / 128, (1L << 30) / 128 + 1}) {
                        const int nout[2] = {128, n1};
                        done("prcnn_mlp_chain_rows_split", prcnn_mlp_chain_rows_split(al ? U(0) : A(0), 128, rows, K, wc, wp, bs, nout, relu, terms, A(4), 136, 8, nullptr));
                    }
    for (int terms : {3, 6})
        for (int B : {0, 1, 8, 16})
            for (int n : {1, 128, 4096, 16384})
                for (int C2 : {128, 64})
                    for (int al = 0; al < 2; al++)
                        for (int m : {64, (1 << 30) / 128 / 16 - 1, (1 << 30) / 128 / 16, (1 << 30) / 128 / 16 + 1, (1 << 30) / 128}) {
                            const int rc = prcnn_mlp_chain_interp_split(al ? U(0) : A(0), 128, AI(1), A(2), B, n, m, C2, A(3), A<void>(10), A(12), A(14), 128, 1, terms, A(4), 128,
                                                                        0, nullptr);
                            done("prcnn_mlp_chain_interp_split", rc);
                        }
}

static void sweep_all() {
    sweep_rows();
    sweep_addinterp();
    sweep_group();
    sweep_interp();
    sweep_chains();
    sweep_split_chains();
}

int main(int argc, char** argv) {
    g_dump = argc > 1 && strcmp(argv[1], "--dump") == 0;
    static const char* const SETTINGS[][2] = {
        {nullptr, nullptr},          {"PRCNN_GROUP_SPLIT", "0"},    {"PRCNN_SPLIT_MIN_TILES", "64"}, {"PRCNN_SPLIT_WIDE_MIN", "1000"}, {"PRCNN_BOUNDED_GRID", "0"},
        {"PRCNN_WIDE_MIN_TILES", "400"}, {"PRCNN_WIDE_LISTS", "1"},  {"PRCNN_LAYER_V1", "1"},         {"PRCNN_NO_WGM", "1"},            {"PRCNN_NO_ROWS32", "1"},
        {"PRCNN_NO_STACK", "1"},     {"PRCNN_NO_SA0", "1"},         {"PRCNN_PERSISTENT_CHAIN", "1"}, {"PRCNN_NO_FAST_CHAIN", "1"},     {"PRCNN_CHAIN_COOP", "0"},
        {"PRCNN_CHAIN_COOP", "1"},   {"PRCNN_CHAIN_COOP", "2"},     {"PRCNN_CHAIN_PERSIST", "0"},    {"PRCNN_NO_XCD_ORDER", "1"},      {"PRCNN_ADDY_PHASE", "0"}};
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    for (const auto& st : SETTINGS) {
        if (st[0]) setenv(st[0], st[1], 1);
        prcnn_switch_reload();
        g_setting = st[0] ? std::string(st[0]) + "=" + st[1] : std::string("default");
        // PRCNN_NO_STACK withdraws the offer and leaves the dispatch as it is: the two disagree under it, by design
        g_check_supported = !(st[0] && strcmp(st[0], "PRCNN_NO_STACK") == 0);
        sweep_all();
        if (st[0]) unsetenv(st[0]);
    }
    long calls = 0;
    for (const Group& g : g_groups) {
        if (!g_dump) printf("%s %ld %016llx\n", g.name.c_str(), g.calls, g.h);
        calls += g.calls;
    }
    printf("%ld calls, %d groups, %d inconsistent\n", calls, (int)g_groups.size(), g_inconsistent);
    return g_inconsistent ? 1 : 0;
}
