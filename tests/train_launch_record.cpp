// Stand-alone host program: which kernel instantiations the training SharedMLP (csrc/mlp_train.h, included at the end of mlp.hip)
// launches for a stack -- recorded, not launched (tests/train_record_common.h).  The pointers are dummies, never dereferenced.
// Built and run by tests/test_train_stack_variants_cpu.py (once plain, once with -fsanitize=address,undefined).
//   train_launch_record --sweep     the universe: every instantiation some call of a broad sweep over rows, widths, sources, pooling,
//                                   padding-free rows, BatchNorm, input gradient and the two native switches launches
//   train_launch_record --case SOURCE ROWS POOL_NS BN NEED_X GENERIC DIRECT K0 N1 [N2 ...]
//                                   one stack as pointrcnn_amd/train_mlp.py would call it.  SOURCE: plain, group, flat (padding-free
//                                   group), interp; ROWS: the host-side row count (flat: B * M * ns); POOL_NS: 0 or nsample
// One line per distinct launch: the kernel instantiation; for the direct wgrad kernel, whose pooling form and operand prologue are
// run-time branches, a second line "train_wgrad_kernel pool=<0 rows | 1 fixed groups | 2 padding-free groups> pro=<0|1>".
//   train_launch_record --digest    the full record, as tests/mlp_launch_record.cpp keeps it for the inference exports: the five stack
//                                   exports and prcnn_train_stack_work_bytes over the union of the three recorders' sweeps, the four
//                                   settings of the two native switches, operand variants that flip every alignment-dependent choice
//                                   and an invalid call per check of the host code (what is crossed with what: digest()).  Per call:
//                                   return code, message, and per launch the
//                                   kernel instantiation, grid, block, dynamic LDS and every argument, parameter structs field by field.
//                                   One line per (switch setting, export, source): number of calls and an FNV-1a digest of their
//                                   records (tests/golden/train_launch_digests.txt); --digest-dump prints every record instead
#include "train_record_common.h"

static std::set<std::string> g_seen;

static void run_case(const Case& c) {
    std::vector<Launch> fwd, bwd;
    run_stack(c, VIA_FP32, fwd, bwd);
    for (const std::vector<Launch>* v : {&fwd, &bwd})
        for (const Launch& x : *v) {
            g_seen.insert(x.name);
            if (!x.tag.empty() && starts(x.name, "train_wgrad_kernel<")) g_seen.insert("train_wgrad_kernel " + x.tag);
        }
}

static void set_switches(bool generic, bool direct) {
    if (generic) setenv("PRCNN_TRAIN_FWD_GENERIC", "1", 1); else unsetenv("PRCNN_TRAIN_FWD_GENERIC");
    if (direct) setenv("PRCNN_WGRAD_DIRECT", "1", 1); else unsetenv("PRCNN_WGRAD_DIRECT");
    prcnn_switch_reload();
}

// f(case): every stack of the sweep -- per (rows, K, N) all sources, pooled / not, BatchNorm / none, input gradient wanted / not;
// three layers: (K, N) from the source, (N, K') and (K', N) behind a BatchNorm + ReLU prologue; one layer
template <class F> static void for_stacks(long rows, int K, int N, F f) {
    for (int source = 0; source < 4; source++)
        for (int pool = 0; pool < 2; pool++)
            for (int bn = 0; bn < 2; bn++)
                for (int need_x = 0; need_x < 2; need_x++) {
                    if ((source == 1 || source == 3) && K < 3) continue;
                    if (source == 3 && !pool) continue;          // padding-free rows are always pooled
                    const int ns = pool ? 16 : 0;
                    const long r = pool ? rows / 16 * 16 : rows;
                    if (r == 0) continue;
                    Case c = {source, r, ns, bn, need_x, 3, {K, N, (K + 3) / 4 * 4, N}};
                    f(c);
                    c.nl = 1;
                    f(c);
                }
}

static void sweep() {
    static const long ROWS[] = {1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096, 6016, 6017, 12160, 12161, 24448, 24449, 100000, 2000000};
    static const int CH[] = {3, 4, 16, 32, 33, 64, 65, 96, 128, 256, 512};
    for (int sw = 0; sw < 4; sw++) {
        set_switches(sw & 1, sw & 2);
        for (long rows : ROWS) {
            if (sw && rows != 129 && rows != 6017 && rows != 100000) continue;          // the switches: a narrow, a wide and a long stack
            for (int K : CH)
                for (int N : CH)
                    if (N % 4 == 0) for_stacks(rows, K, N, run_case);          // (an output width must be a multiple of 4)
        }
    }
}

// ---- --digest ---------------------------------------------------------------------------------------------------------------
struct Group { std::string name; long calls = 0; unsigned long long h = 1469598103934665603ull; };
static std::vector<Group> g_groups;
static bool g_dump = false;
static std::string g_setting;
static const char* const SOURCES[] = {"plain", "group", "interp", "flat"};
static const char* const EXPORTS[] = {"prcnn_train_stack_fwd", "prcnn_train_stack_fwd_split", "prcnn_train_stack_bwd", "prcnn_train_stack_bwd_split",
                                      "prcnn_train_stack_bwd_wsplit"};

// ends a call: files its record (g_rec: message and launches) under (setting, export, source)
static void done(const char* exp, const char* source, int rc) {
    const std::string key = g_setting + " " + exp + " " + source;
    size_t gi = g_groups.size();
    while (gi > 0 && g_groups[gi - 1].name != key) gi--;          // (the group of the last call, most of the time)
    if (gi == 0) { g_groups.push_back({key}); gi = g_groups.size(); }
    Group& g = g_groups[gi - 1];
    char head[64];
    snprintf(head, sizeof head, "#%ld rc %d", g.calls, rc);
    for (const char* p = head; *p; p++) g.h = (g.h ^ (unsigned char)*p) * 1099511628211ull;
    for (unsigned char ch : g_rec) g.h = (g.h ^ ch) * 1099511628211ull;
    g.h = (g.h ^ '\n') * 1099511628211ull;
    g.calls++;
    if (g_dump) printf("%s %s%s\n", key.c_str(), head, g_rec.c_str());
    g_rec.clear();
    g_launches = 0;
}

// the five exports on one stack (which: bit e = EXPORTS[e]); each call on its own, a backward pass does not wait for a forward
static void call_exports(const Stack& s, const char* source, int which = 31) {
    if (which & 1) done(EXPORTS[0], source, call_fwd(s, VIA_FP32));
    if (which & 2) done(EXPORTS[1], source, call_fwd(s, VIA_SPLIT));
    if (which & 4) done(EXPORTS[2], source, call_bwd(s, VIA_FP32));
    if (which & 8) done(EXPORTS[3], source, call_bwd(s, VIA_SPLIT));
    if (which & 16) done(EXPORTS[4], source, call_bwd(s, VIA_WSPLIT));
}
static void work_bytes(const char* source, int64_t rows, const prcnn_train_layer_t* L, int nl, int K0) {
    for (int backward = 0; backward < 2; backward++) {
        recf(" bytes %zu", prcnn_train_stack_work_bytes(rows, L, nl, K0, backward));
        done("prcnn_train_stack_work_bytes", source, 0);
    }
}

template <class T> static T* off(T* p, int bytes) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + bytes); }

static void digest_case(const Case& c, int which, bool variants) {
    const char* source = SOURCES[c.source];
    Stack s;
    build_stack(c, s);
    work_bytes(source, s.S.rows, s.L, s.nl, s.S.K);
    call_exports(s, source, which);
    if (!variants) return;
    // the alignment-dependent choices: vector loads and the fast / split forward of plain rows, the LDS-staged / split wgrad of layer 0
    if (c.source == 0) {
        Stack v = s;
        v.S.in = off(s.S.in, 4);                                    // (the backward pass refuses it: 8-byte rows)
        call_exports(v, source);
        v = s;
        v.S.ld_in = s.S.ld_in + 2;
        call_exports(v, source);
    } else {
        Stack v = s;
        v.dump = off(s.dump, 8);                                    // (the forward pass refuses it: 16-byte rows)
        call_exports(v, source);
        v = s;
        v.ldd = s.ldd + 2;
        call_exports(v, source, 4 | 8 | 16);
    }
    Stack v = s;                                                    // a split image for some layers only
    for (int l = 0; l < s.nl; l++) (l % 2 ? v.ws : v.wst)[l] = nullptr;
    call_exports(v, source, 2 | 8 | 16);
    for (int l = 0; l < s.nl; l++) { v.ws[l] = l % 2 ? s.ws[l] : nullptr; v.wst[l] = l % 2 ? nullptr : s.wst[l]; }
    call_exports(v, source, 2 | 8 | 16);
}

// an invalid call per check of the host code, each one edit away from a valid stack; filed under the source "invalid"
static void digest_invalid() {
    const Case BASE[4] = {{0, 6016, 0, 1, 1, 3, {64, 128, 64, 128}}, {1, 6016, 16, 1, 1, 3, {67, 128, 64, 128}}, {2, 6016, 0, 1, 1, 3, {64, 128, 64, 128}},
                          {3, 6016, 16, 1, 1, 3, {67, 128, 64, 128}}};
    Stack b[4];
    for (int i = 0; i < 4; i++) build_stack(BASE[i], b[i]);
    auto bad = [&](int base, int which, auto edit) {
        Stack v = b[base];
        edit(v);
        call_exports(v, "invalid", which);
    };
    const int FWD = 1 | 2, BWD = 4 | 8 | 16, ALL = 31;
    // the source descriptor (forward only: the backward pass reads the descriptor the forward pass checked)
    bad(0, ALL, [](Stack& v) { v.S.rows = 0; });
    bad(0, ALL, [](Stack& v) { v.S.K = 0; });
    bad(0, ALL, [](Stack& v) { v.S.in = nullptr; });
    bad(0, ALL, [](Stack& v) { v.S.ld_in = v.S.K - 4; });
    bad(1, FWD, [](Stack& v) { v.S.xyz = nullptr; });
    bad(1, FWD, [](Stack& v) { v.S.idx = nullptr; });
    bad(1, FWD, [](Stack& v) { v.S.feat = nullptr; });
    bad(1, FWD, [](Stack& v) { v.S.C = v.S.K; });
    bad(1, FWD, [](Stack& v) { v.S.M++; });
    bad(1, FWD, [](Stack& v) { v.S.N = 0; });
    bad(2, FWD, [](Stack& v) { v.S.known = nullptr; });
    bad(2, FWD, [](Stack& v) { v.S.skip = nullptr; });
    bad(2, FWD, [](Stack& v) { v.S.C2++; });
    bad(2, FWD, [](Stack& v) { v.S.n++; });
    bad(2, FWD, [](Stack& v) { v.S.m = 0; });
    bad(0, ALL, [](Stack& v) { v.S.mode = 7; });
    // the layers
    bad(0, ALL, [](Stack& v) { v.nl = 0; });
    bad(0, ALL, [](Stack& v) { v.nl = 9; });
    bad(0, ALL, [](Stack& v) { v.L[1].Nout = 66; });
    bad(0, ALL, [](Stack& v) { v.L[2].Nout = 0; });
    bad(0, ALL, [](Stack& v) { v.L[0].W = nullptr; });
    bad(0, ALL, [](Stack& v) { v.L[1].y = nullptr; });
    bad(0, ALL, [](Stack& v) { v.L[2].cst = nullptr; });
    bad(0, ALL, [](Stack& v) { v.L[0].wpack = nullptr; });
    bad(0, ALL, [](Stack& v) { v.L[0].ld_c = 192; });
    bad(0, ALL, [](Stack& v) { v.L[1].ld_c = 0; });
    bad(0, ALL, [](Stack& v) { v.L[1].cst = off(v.L[1].cst, 4); });
    bad(0, ALL, [](Stack& v) { v.L[2].y = off(v.L[2].y, 8); });
    bad(0, ALL, [](Stack& v) { v.L[0].wpack = off(v.L[0].wpack, 4); });
    // padding-free rows
    bad(0, ALL, [](Stack& v) { v.S.mult = A(5); });
    bad(3, ALL, [](Stack& v) { v.S.rows_dev = nullptr; });
    bad(3, ALL, [](Stack& v) { v.S.seg_off = nullptr; });
    bad(3, ALL, [](Stack& v) { v.S.seg_cnt = nullptr; });
    bad(3, ALL, [](Stack& v) { v.S.row_grp = nullptr; });
    bad(3, ALL, [](Stack& v) { v.S.groups = 0; });
    bad(3, ALL, [](Stack& v) { v.S.norm_rows = 0; });
    bad(3, ALL, [](Stack& v) { v.arg = nullptr; });
    // pooling, the output, the gradient
    bad(1, ALL, [](Stack& v) { v.out = nullptr; v.gout = nullptr; });
    bad(1, ALL, [](Stack& v) { v.ns = 256; });
    bad(1, ALL, [](Stack& v) { v.ns = 17; });
    bad(1, ALL, [](Stack& v) { v.arg = nullptr; });
    bad(0, ALL, [](Stack& v) { v.ld_out += 2; v.ld_gout += 2; });
    bad(0, ALL, [](Stack& v) { v.col_off = 2; });
    bad(0, ALL, [](Stack& v) { v.out = off(v.out, 4); v.gout = off(v.gout, 4); });
    bad(0, FWD, [](Stack& v) { v.col_off = 4; });
    // the assembled rows of a gathered source, the first layer's input rows, the prologue
    bad(0, FWD, [](Stack& v) { v.dump = A(10); v.ldd = 64; });
    bad(1, ALL, [](Stack& v) { v.dump = off(v.dump, 4); });
    bad(1, ALL, [](Stack& v) { v.ldd = 64; });
    bad(1, ALL, [](Stack& v) { v.ldd = 69; });
    bad(2, BWD, [](Stack& v) { v.dump = nullptr; });
    bad(0, BWD, [](Stack& v) { v.S.ld_in = 65; });
    bad(0, FWD, [](Stack& v) { v.S.pro_scale = A(15); });
    bad(0, FWD, [](Stack& v) { v.S.pro_shift = A(16); });
    // the input gradient
    bad(0, BWD, [](Stack& v) { v.ld_gin = 60; });
    bad(0, BWD, [](Stack& v) { v.L[0].wpack_t = nullptr; });
    bad(1, BWD, [](Stack& v) { v.S.K = 3; v.S.C = 0; v.ldd = 4; });
    // the workspace
    bad(0, ALL, [](Stack& v) { v.work = nullptr; });
    bad(0, ALL, [](Stack& v) { v.work = off(v.work, 128); });
    bad(0, FWD, [](Stack& v) { v.work_bytes = prcnn_train_stack_work_bytes(v.S.rows, v.L, v.nl, v.S.K, 0) - 1; });
    bad(0, BWD, [](Stack& v) { v.work_bytes = prcnn_train_stack_work_bytes(v.S.rows, v.L, v.nl, v.S.K, 1) - 1; });
    // inside the loops (the layers before the failing one have launched): gradient outputs, the transposed weights, the split images
    bad(0, BWD, [](Stack& v) { v.L[2].dW = nullptr; });
    bad(0, BWD, [](Stack& v) { v.L[0].dW = nullptr; });
    bad(0, BWD, [](Stack& v) { v.L[1].dgamma = nullptr; });
    bad(0, BWD, [](Stack& v) { v.L[1].dbeta = nullptr; });
    bad(0, BWD, [](Stack& v) { v.L[1].wpack_t = nullptr; });
    bad(0, BWD, [](Stack& v) { v.L[2].wpack_t = nullptr; });
    bad(0, 2, [](Stack& v) { v.ws[0] = off(v.ws[0], 8); });
    bad(0, 2, [](Stack& v) { v.ws[2] = off(v.ws[2], 4); });
    bad(0, 8 | 16, [](Stack& v) { v.wst[2] = off(v.wst[2], 8); });
    bad(0, 8 | 16, [](Stack& v) { v.wst[0] = off(v.wst[0], 4); });
    // null descriptors and tables
    const Stack& s = b[0];
    done(EXPORTS[0], "invalid", prcnn_train_stack_fwd(nullptr, s.L, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, 0, s.arg, s.work, s.work_bytes, nullptr));
    done(EXPORTS[0], "invalid", prcnn_train_stack_fwd(&s.S, nullptr, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, 0, s.arg, s.work, s.work_bytes, nullptr));
    done(EXPORTS[1], "invalid", prcnn_train_stack_fwd_split(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, 0, s.arg, nullptr, s.work, s.work_bytes, nullptr));
    done(EXPORTS[2], "invalid", prcnn_train_stack_bwd(nullptr, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.work, s.work_bytes, nullptr));
    done(EXPORTS[2], "invalid", prcnn_train_stack_bwd(&s.S, nullptr, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.work, s.work_bytes, nullptr));
    done(EXPORTS[3], "invalid", prcnn_train_stack_bwd_split(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, nullptr, s.work, s.work_bytes, nullptr));
    done(EXPORTS[4], "invalid", prcnn_train_stack_bwd_wsplit(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, nullptr, s.work, s.work_bytes, nullptr));
    work_bytes("invalid", s.S.rows, nullptr, s.nl, s.S.K);
    work_bytes("invalid", s.S.rows, s.L, 0, s.S.K);
    work_bytes("invalid", 0, s.L, s.nl, s.S.K);
}

static int digest() {
    // the union of the three recorders' sweeps (this file's, train_split_launch_record.cpp's, train_wsplit_launch_record.cpp's)
    static const long ROWS[] = {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025, 4096, 6016, 6017, 12160, 12161, 24448, 24449, 100000, 2000000};
    static const int CH[] = {3, 4, 16, 32, 33, 64, 65, 68, 96, 128, 132, 196, 256, 512, 515};
    static const char* const SETTINGS[] = {"default", "PRCNN_TRAIN_FWD_GENERIC=1", "PRCNN_WGRAD_DIRECT=1", "PRCNN_TRAIN_FWD_GENERIC=1,PRCNN_WGRAD_DIRECT=1"};
    g_fields = true;
    for (int sw = 0; sw < 4; sw++) {
        set_switches(sw & 1, sw & 2);
        g_setting = SETTINGS[sw];
        // a switch: the exports it bears on (forward: PRCNN_TRAIN_FWD_GENERIC, backward: PRCNN_WGRAD_DIRECT)
        const int which = sw == 1 ? 1 | 2 : sw == 2 ? 4 | 8 | 16 : 31;
        for (long rows : ROWS) {
            // a narrow, a wide and a long stack take the switches, the operand variants and every pair of BatchNorm x input gradient;
            // the other rows: both or neither
            const bool few = rows == 129 || rows == 6017 || rows == 100000;
            if (sw && !few) continue;
            for (int K : CH)
                for (int N : CH)
                    if (N % 4 == 0 && N <= 512)
                        for_stacks(rows, K, N, [&](const Case& c) { if (few || c.bn == c.need_x) digest_case(c, which, few && !sw); });
        }
        digest_invalid();
    }
    long calls = 0;
    for (const Group& g : g_groups) {
        if (!g_dump) printf("%s %ld %016llx\n", g.name.c_str(), g.calls, g.h);
        calls += g.calls;
    }
    printf("%ld calls, %d groups\n", calls, (int)g_groups.size());
    return 0;
}

int main(int argc, char** argv) {
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    Case c;
    if (argc > 1 && (strcmp(argv[1], "--digest") == 0 || strcmp(argv[1], "--digest-dump") == 0)) {
        g_dump = strcmp(argv[1], "--digest-dump") == 0;
        return digest();
    } else if (argc > 1 && strcmp(argv[1], "--sweep") == 0) {
        sweep();
    } else if (argc >= 11 && strcmp(argv[1], "--case") == 0) {
        if (!parse_case(argc, argv, 2, 2, c)) return 2;
        set_switches(atoi(argv[7]) != 0, atoi(argv[8]) != 0);
        run_case(c);
    } else {
        fprintf(stderr, "usage: train_launch_record --sweep | --digest | --case SOURCE ROWS POOL_NS BN NEED_X GENERIC DIRECT K0 N1 [N2 ...]\n");
        return 2;
    }
    for (const std::string& s : g_seen) printf("%s\n", s.c_str());
    return g_failed ? 1 : 0;
}
