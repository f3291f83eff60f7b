// Stand-alone host program: which kernel instantiations the training SharedMLP (csrc/mlp_train.h, included at the end of mlp.hip)
// launches for a stack -- recorded, not launched (tests/launch_record_prelude.h).  The pointers are dummies, never dereferenced.
// Built and run by tests/test_train_stack_variants_cpu.py (once plain, once with -fsanitize=address,undefined).
//   train_launch_record --sweep     the universe: every instantiation some call of a broad sweep over rows, widths, sources, pooling,
//                                   padding-free rows, BatchNorm, input gradient and the two native switches launches
//   train_launch_record --case SOURCE ROWS POOL_NS BN NEED_X GENERIC DIRECT K0 N1 [N2 ...]
//                                   one stack as pointrcnn_amd/train_mlp.py would call it.  SOURCE: plain, group, flat (padding-free
//                                   group), interp; ROWS: the host-side row count (flat: B * M * ns); POOL_NS: 0 or nsample
// One line per distinct launch: the kernel instantiation; for the direct wgrad kernel, whose pooling form and operand prologue are
// run-time branches, a second line "train_wgrad_kernel pool=<0 rows | 1 fixed groups | 2 padding-free groups> pro=<0|1>".
#include "launch_record_prelude.h"
#include <cxxabi.h>
#include <set>
struct TrainWgrad;
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const TrainWgrad& W);

#ifndef MLP_SOURCE
#define MLP_SOURCE "mlp.hip"
#endif
#include MLP_SOURCE

static void rec_params(const MlpParams&) {}
static void rec_params(const ChainParams&) {}
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const TrainWgrad& W) {
    rec_head(k, g, b, lds);
    recf(" ~pool=%d pro=%d", W.B.pool_ns == 0 ? 0 : W.B.pool_ns > 0 ? 1 : 2, W.pro_scale ? 1 : 0);
}

template <class T = float> static T* A(int i) { return reinterpret_cast<T*>((uintptr_t)0x100000 * (i + 1)); }

static std::set<std::string> g_seen;
static int g_failed = 0;

// "KName<&train_wgrad_kernel<1, 1, 1, 1>(TrainWgrad)>" or "KName<&(void train_x<...>(T))>" -> "train_wgrad_kernel<1, 1, 1, 1>"
static std::string pretty(const std::string& mangled) {
    int st = 0;
    char* d = abi::__cxa_demangle(mangled.c_str(), nullptr, nullptr, &st);
    std::string s = (st == 0 && d) ? d : mangled;
    free(d);
    const size_t amp = s.find('&');
    const size_t par = s.rfind('(');
    if (amp == std::string::npos || par == std::string::npos || par <= amp) return s;
    s = s.substr(amp + 1, par - amp - 1);
    if (s.compare(0, 1, "(") == 0) s.erase(0, 1);
    if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
    return s;
}

// files the launches of the call in flight
static void harvest(int rc) {
    if (rc != PRCNN_OK) { g_failed++; fprintf(stderr, "call failed (%d):%s\n", rc, g_rec.c_str()); }
    size_t p = 0;
    while ((p = g_rec.find(" | ", p)) != std::string::npos) {
        p += 3;
        const size_t e = g_rec.find(" grid ", p);
        if (e == std::string::npos) break;
        const std::string name = pretty(g_rec.substr(p, e - p));
        g_seen.insert(name);
        const size_t nxt = g_rec.find(" | ", e);
        const size_t tag = g_rec.find(" ~", e);
        if (tag != std::string::npos && (nxt == std::string::npos || tag < nxt) && name.compare(0, 19, "train_wgrad_kernel<") == 0)
            g_seen.insert("train_wgrad_kernel " + g_rec.substr(tag + 2, (nxt == std::string::npos ? g_rec.size() : nxt) - tag - 2));
    }
    g_rec.clear();
    g_launches = 0;
}

struct Case { int source; long rows; int pool_ns, bn, need_x, nl; int chans[9]; };          // source: 0 plain, 1 group, 2 interp, 3 flat

static void run_case(const Case& c) {
    prcnn_train_src_t S = {};
    const int K0 = c.chans[0];
    S.rows = c.rows; S.K = K0;
    const int ns = c.pool_ns > 1 ? c.pool_ns : 1;
    if (c.source == 0) {
        S.mode = MODE_PLAIN; S.in = A(0); S.ld_in = (K0 + 3) / 4 * 4;
    } else if (c.source == 1) {
        S.mode = MODE_GROUP; S.xyz = A(1); S.new_xyz = A(2); S.idx = A<int32_t>(3); S.feat = K0 > 3 ? A(4) : nullptr; S.ld_feat = (K0 - 3 + 3) / 4 * 4;
        S.B = 1; S.N = 4096; S.M = (int)(c.rows / ns); S.ns = ns; S.C = K0 - 3;
    } else if (c.source == 3) {
        S.mode = MODE_GROUP; S.xyz = A(1); S.new_xyz = A(2); S.idx = A<int32_t>(3); S.feat = K0 > 3 ? A(4) : nullptr; S.ld_feat = (K0 - 3 + 3) / 4 * 4;
        S.B = 1; S.N = 4096; S.M = (int)c.rows; S.ns = 1; S.C = K0 - 3;
        S.mult = A(5); S.rows_dev = A<int32_t>(6); S.norm_rows = c.rows; S.seg_off = A<int32_t>(7); S.seg_cnt = A<int32_t>(8); S.row_grp = A<int32_t>(9);
        S.groups = (int)(c.rows / ns);
    } else {
        S.mode = MODE_INTERP; S.known = A(1); S.idx3 = A<int32_t>(2); S.w3 = A(3);
        S.C1 = K0 > 4 ? K0 / 4 : 0; S.C2 = K0 - S.C1;
        S.skip = S.C1 ? A(4) : nullptr; S.ld_known = (S.C2 + 3) / 4 * 4; S.ld_skip = (S.C1 + 3) / 4 * 4;
        S.B = 1; S.n = (int)c.rows; S.m = 64;
    }
    prcnn_train_layer_t L[8] = {};
    for (int l = 0; l < c.nl; l++) {
        L[l].Nout = c.chans[l + 1];
        L[l].W = A(20 + l); L[l].y = A(30 + l); L[l].cst = A(40 + l); L[l].ld_c = (L[l].Nout + 127) / 128 * 128; L[l].wpack = A(50 + l);
        L[l].wpack_t = (l > 0 || (c.need_x && (c.source == 1 || c.source == 3 ? K0 - 3 : K0) > 0)) ? A(60 + l) : nullptr;
        L[l].dW = A(70 + l);
        if (c.bn) { L[l].gamma = A(80 + l); L[l].beta = A(90 + l); L[l].dgamma = A(100 + l); L[l].dbeta = A(110 + l); L[l].running_mean = A(120 + l); L[l].running_var = A(130 + l); }
        else if (l % 2 == 0) { L[l].beta = A(90 + l); L[l].dbeta = A(110 + l); }          // Conv with bias / without, alternating
        L[l].eps = 1e-5f; L[l].momentum = 0.1f;
    }
    const int kin0 = (c.source == 1 || c.source == 3) ? K0 - 3 : K0;
    const bool need_x = c.need_x && kin0 > 0;
    const bool gathered = c.source != 0;
    const int ld_dump = (K0 + 3) / 4 * 4;
    void* work = A<void>(200);
    const int pool_arg = ns;
    const bool has_arg = ns > 1 || c.source == 3;
    const int rc = prcnn_train_stack_fwd(&S, L, c.nl, pool_arg, gathered ? A(10) : nullptr, gathered ? ld_dump : 0, A(11), c.chans[c.nl], 0,
                                         has_arg ? A<uint8_t>(12) : nullptr, work, (size_t)1 << 62, nullptr);
    harvest(rc);
    if (rc != PRCNN_OK) return;                                   // (no backward without a forward)
    harvest(prcnn_train_stack_bwd(&S, L, c.nl, pool_arg, gathered ? A(10) : nullptr, gathered ? ld_dump : 0, A(13), c.chans[c.nl],
                                  has_arg ? A<uint8_t>(12) : nullptr, need_x ? A(14) : nullptr, need_x ? (kin0 + 3) / 4 * 4 : 0, work, (size_t)1 << 62,
                                  nullptr));
}

static void set_switches(bool generic, bool direct) {
    if (generic) setenv("PRCNN_TRAIN_FWD_GENERIC", "1", 1); else unsetenv("PRCNN_TRAIN_FWD_GENERIC");
    if (direct) setenv("PRCNN_WGRAD_DIRECT", "1", 1); else unsetenv("PRCNN_WGRAD_DIRECT");
    prcnn_switch_reload();
}

static void sweep() {
    static const long ROWS[] = {1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096, 6016, 6017, 12160, 12161, 24448, 24449, 100000, 2000000};
    static const int CH[] = {3, 4, 16, 32, 33, 64, 65, 96, 128, 256, 512};
    for (int sw = 0; sw < 4; sw++) {
        set_switches(sw & 1, sw & 2);
        for (long rows : ROWS) {
            if (sw && rows != 129 && rows != 6017 && rows != 100000) continue;          // the switches: a narrow, a wide and a long stack
            for (int K : CH)
                for (int N : CH) {
                    if (N % 4) continue;                              // (an output width must be a multiple of 4)
                    for (int source = 0; source < 4; source++)
                        for (int pool = 0; pool < 2; pool++)
                            for (int bn = 0; bn < 2; bn++)
                                for (int need_x = 0; need_x < 2; need_x++) {
                                    if ((source == 1 || source == 3) && K < 3) continue;
                                    if (source == 3 && !pool) continue;          // padding-free rows are always pooled
                                    const int ns = pool ? 16 : 0;
                                    const long r = pool ? rows / 16 * 16 : rows;
                                    if (r == 0) continue;
                                    // three layers: (K, N) from the source, (N, K') and (K', N) behind a BatchNorm + ReLU prologue; one layer
                                    Case c = {source, r, ns, bn, need_x, 3, {K, N, (K + 3) / 4 * 4, N}};
                                    run_case(c);
                                    c.nl = 1;
                                    run_case(c);
                                }
                }
        }
    }
}

int main(int argc, char** argv) {
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    if (argc > 1 && strcmp(argv[1], "--sweep") == 0) {
        sweep();
    } else if (argc >= 11 && strcmp(argv[1], "--case") == 0) {
        Case c = {};
        const std::string src = argv[2];
        c.source = src == "plain" ? 0 : src == "group" ? 1 : src == "interp" ? 2 : src == "flat" ? 3 : -1;
        if (c.source < 0) { fprintf(stderr, "unknown source %s\n", argv[2]); return 2; }
        c.rows = atol(argv[3]); c.pool_ns = atoi(argv[4]); c.bn = atoi(argv[5]); c.need_x = atoi(argv[6]);
        set_switches(atoi(argv[7]) != 0, atoi(argv[8]) != 0);
        c.nl = argc - 10;
        if (c.nl > 8) { fprintf(stderr, "at most 8 layers\n"); return 2; }
        for (int i = 0; i <= c.nl; i++) c.chans[i] = atoi(argv[9 + i]);
        run_case(c);
    } else {
        fprintf(stderr, "usage: train_launch_record --sweep | --case SOURCE ROWS POOL_NS BN NEED_X GENERIC DIRECT K0 N1 [N2 ...]\n");
        return 2;
    }
    for (const std::string& s : g_seen) printf("%s\n", s.c_str());
    return g_failed ? 1 : 0;
}
