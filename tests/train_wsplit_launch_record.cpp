// Stand-alone host program: which wgrad kernel every layer of a training SharedMLP gets through prcnn_train_stack_bwd_wsplit
// (csrc/mlp_train.h) -- recorded, not launched (tests/launch_record_prelude.h), as tests/train_split_launch_record.cpp does for the
// split forward / dgrad entry points.  The pointers are dummies, never dereferenced; every layer is offered a split image for its
// dgrad as well, so the library's own eligibility rules decide.
// Built and run by tests/test_train_wsplit_cpu.py (once plain, once with -fsanitize=address,undefined).
//   train_wsplit_launch_record --sweep VIA   every kernel a broad sweep launches; VIA = wsplit (prcnn_train_stack_fwd_split +
//                                            _bwd_wsplit), split (_fwd_split + _bwd_split) or fp32 (prcnn_train_stack_fwd + _bwd)
//   train_wsplit_launch_record --case VIA SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]
//                                            one stack: "wgrad <layer> <kernel>" per layer in layer order, "also <kernel>" for every
//                                            other distinct launch of the backward pass
#include "launch_record_prelude.h"
#include <cxxabi.h>
#include <set>

#ifndef MLP_SOURCE
#define MLP_SOURCE "mlp.hip"
#endif
#include MLP_SOURCE

static void rec_params(const MlpParams&) {}
static void rec_params(const ChainParams&) {}

template <class T = float> static T* A(int i) { return reinterpret_cast<T*>((uintptr_t)0x100000 * (i + 1)); }

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

static int g_failed = 0;

// the kernel names of the call in flight, in order
static std::vector<std::string> harvest(int rc) {
    std::vector<std::string> out;
    if (rc != PRCNN_OK) { g_failed++; fprintf(stderr, "call failed (%d):%s\n", rc, g_rec.c_str()); }
    size_t p = 0;
    while ((p = g_rec.find(" | ", p)) != std::string::npos) {
        p += 3;
        const size_t e = g_rec.find(" grid ", p);
        if (e == std::string::npos) break;
        out.push_back(pretty(g_rec.substr(p, e - p)));
    }
    g_rec.clear();
    g_launches = 0;
    return out;
}

enum Via { VIA_FP32 = 0, VIA_SPLIT = 1, VIA_WSPLIT = 2 };
struct Case { int source; long rows; int pool_ns, bn, need_x, nl; int chans[9]; };          // source: 0 plain, 1 group, 2 interp, 3 flat

// the descriptors of tests/train_split_launch_record.cpp's run_case; the launches of the backward pass
static std::vector<std::string> run_case(const Case& c, int via) {
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
    void* ws[8];
    void* wst[8];
    for (int l = 0; l < c.nl; l++) {
        L[l].Nout = c.chans[l + 1];
        L[l].W = A(20 + l); L[l].y = A(30 + l); L[l].cst = A(40 + l); L[l].ld_c = (L[l].Nout + 127) / 128 * 128; L[l].wpack = A(50 + l);
        L[l].wpack_t = (l > 0 || (c.need_x && (c.source == 1 || c.source == 3 ? K0 - 3 : K0) > 0)) ? A(60 + l) : nullptr;
        L[l].dW = A(70 + l);
        if (c.bn) { L[l].gamma = A(80 + l); L[l].beta = A(90 + l); L[l].dgamma = A(100 + l); L[l].dbeta = A(110 + l); L[l].running_mean = A(120 + l); L[l].running_var = A(130 + l); }
        else if (l % 2 == 0) { L[l].beta = A(90 + l); L[l].dbeta = A(110 + l); }          // Conv with bias / without, alternating
        L[l].eps = 1e-5f; L[l].momentum = 0.1f;
        ws[l] = A<void>(140 + l); wst[l] = A<void>(150 + l);
    }
    const int kin0 = (c.source == 1 || c.source == 3) ? K0 - 3 : K0;
    const bool need_x = c.need_x && kin0 > 0;
    const bool gathered = c.source != 0;
    const int ld_dump = (K0 + 3) / 4 * 4;
    void* work = A<void>(200);
    const bool has_arg = ns > 1 || c.source == 3;
    float* dump = gathered ? A(10) : nullptr;
    uint8_t* arg = has_arg ? A<uint8_t>(12) : nullptr;
    const int ldd = gathered ? ld_dump : 0, nlast = c.chans[c.nl], ld_gin = need_x ? (kin0 + 3) / 4 * 4 : 0;
    float* gin = need_x ? A(14) : nullptr;
    int rc;
    if (via == VIA_FP32) rc = prcnn_train_stack_fwd(&S, L, c.nl, ns, dump, ldd, A(11), nlast, 0, arg, work, (size_t)1 << 62, nullptr);
    else rc = prcnn_train_stack_fwd_split(&S, L, c.nl, ns, dump, ldd, A(11), nlast, 0, arg, ws, work, (size_t)1 << 62, nullptr);
    (void)harvest(rc);
    if (rc != PRCNN_OK) return {};                                // (no backward without a forward)
    if (via == VIA_FP32) rc = prcnn_train_stack_bwd(&S, L, c.nl, ns, dump, ldd, A(13), nlast, arg, gin, ld_gin, work, (size_t)1 << 62, nullptr);
    else if (via == VIA_SPLIT) rc = prcnn_train_stack_bwd_split(&S, L, c.nl, ns, dump, ldd, A(13), nlast, arg, gin, ld_gin, wst, work, (size_t)1 << 62, nullptr);
    else rc = prcnn_train_stack_bwd_wsplit(&S, L, c.nl, ns, dump, ldd, A(13), nlast, arg, gin, ld_gin, wst, work, (size_t)1 << 62, nullptr);
    return harvest(rc);
}

static bool starts(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

static void sweep(int via) {
    static const long ROWS[] = {1, 2, 15, 16, 17, 31, 32, 33, 64, 127, 128, 129, 511, 512, 513, 1025, 4096, 6017, 24449, 100000, 2000000};
    static const int CH[] = {3, 4, 16, 32, 33, 64, 65, 68, 96, 128, 132, 196, 256, 512, 515};
    std::set<std::string> seen;
    for (long rows : ROWS)
        for (int K : CH)
            for (int N : CH) {
                if (N % 4 || N > 512) continue;                   // (an output width must be a multiple of 4)
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
                                for (int nl = 3; nl >= 1; nl -= 2) {
                                    c.nl = nl;
                                    for (const std::string& x : run_case(c, via)) seen.insert(x);
                                }
                            }
            }
    for (const std::string& s : seen) printf("%s\n", s.c_str());
}

static int via_of(const char* s) {
    return strcmp(s, "wsplit") == 0 ? VIA_WSPLIT : strcmp(s, "split") == 0 ? VIA_SPLIT : strcmp(s, "fp32") == 0 ? VIA_FP32 : -1;
}

int main(int argc, char** argv) {
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    prcnn_switch_reload();
    const int via = argc > 2 ? via_of(argv[2]) : -1;
    if (argc == 3 && strcmp(argv[1], "--sweep") == 0 && via >= 0) {
        sweep(via);
    } else if (argc >= 10 && strcmp(argv[1], "--case") == 0 && via >= 0) {
        Case c = {};
        const std::string src = argv[3];
        c.source = src == "plain" ? 0 : src == "group" ? 1 : src == "interp" ? 2 : src == "flat" ? 3 : -1;
        if (c.source < 0) { fprintf(stderr, "unknown source %s\n", argv[3]); return 2; }
        c.rows = atol(argv[4]); c.pool_ns = atoi(argv[5]); c.bn = atoi(argv[6]); c.need_x = atoi(argv[7]);
        c.nl = argc - 9;
        if (c.nl > 8) { fprintf(stderr, "at most 8 layers\n"); return 2; }
        for (int i = 0; i <= c.nl; i++) c.chans[i] = atoi(argv[8 + i]);
        // a layer's wgrad follows its BatchNorm backward reductions, last layer first
        std::vector<std::string> wgrad(c.nl);
        std::set<std::string> also;
        int l = c.nl;
        for (const std::string& x : run_case(c, via)) {
            if (starts(x, "bn_bwd_reduce_kernel")) l--;
            if (starts(x, "train_wgrad_") && !starts(x, "train_wgrad_reduce_kernel")) {
                if (l < 0 || l >= c.nl || !wgrad[l].empty()) { fprintf(stderr, "unexpected wgrad launch %s\n", x.c_str()); return 1; }
                wgrad[l] = x;
            } else also.insert(x);
        }
        for (int i = 0; i < c.nl; i++) printf("wgrad %d %s\n", i, wgrad[i].c_str());
        for (const std::string& s : also) printf("also %s\n", s.c_str());
    } else {
        fprintf(stderr, "usage: train_wsplit_launch_record --sweep VIA | --case VIA SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]   (VIA: wsplit, split, fp32)\n");
        return 2;
    }
    return g_failed ? 1 : 0;
}
