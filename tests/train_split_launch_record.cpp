// Stand-alone host program: which kernel instantiations the training SharedMLP launches through the split-bf16 entry points
// (prcnn_train_stack_fwd_split / _bwd_split, csrc/mlp_train.h) -- recorded, not launched (tests/launch_record_prelude.h), as
// tests/train_launch_record.cpp does for the fp32 entry points.  The pointers are dummies, never dereferenced; every layer is
// offered a split image, so the library's own eligibility rules decide.
// Built and run by tests/test_train_split_cpu.py (once plain, once with -fsanitize=address,undefined).
//   train_split_launch_record --sweep        every instantiation a broad sweep through the split entry points launches
//   train_split_launch_record --case SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]
//                                            one stack through the split entry points: "fwd <layer> <kernel>" per forward GEMM in
//                                            layer order, "dgrad <layer> <kernel>" per dgrad GEMM, "also <kernel>" for every other
//                                            distinct launch
//   train_split_launch_record --fp32-case SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]
//                                            the same stack through prcnn_train_stack_fwd / _bwd: one line per launch, in order,
//                                            "<kernel> grid x,y,z block x,y,z" (compared with tests/golden/train_stack_fp32_launches.txt,
//                                            recorded before the split entry points existed)
// TRAIN_SPLIT_RECORD_FP32_ONLY: builds without the split entry points (how the golden file was recorded from the older source).
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

struct Launch { std::string name, shape; };
static int g_failed = 0;

// the launches of the call in flight, in order
static std::vector<Launch> harvest(int rc) {
    std::vector<Launch> out;
    if (rc != PRCNN_OK) { g_failed++; fprintf(stderr, "call failed (%d):%s\n", rc, g_rec.c_str()); }
    size_t p = 0;
    while ((p = g_rec.find(" | ", p)) != std::string::npos) {
        p += 3;
        const size_t e = g_rec.find(" grid ", p);
        if (e == std::string::npos) break;
        size_t end = g_rec.find(" lds ", e);
        if (end == std::string::npos) end = g_rec.size();
        out.push_back({pretty(g_rec.substr(p, e - p)), g_rec.substr(e + 1, end - e - 1)});
    }
    g_rec.clear();
    g_launches = 0;
    return out;
}

struct Case { int source; long rows; int pool_ns, bn, need_x, nl; int chans[9]; };          // source: 0 plain, 1 group, 2 interp, 3 flat

// the descriptors of tests/train_launch_record.cpp's run_case, through either pair of entry points
static void run_case(const Case& c, bool split, std::vector<Launch>& fwd, std::vector<Launch>& bwd) {
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
#ifndef TRAIN_SPLIT_RECORD_FP32_ONLY
    if (split) rc = prcnn_train_stack_fwd_split(&S, L, c.nl, ns, dump, ldd, A(11), nlast, 0, arg, ws, work, (size_t)1 << 62, nullptr);
    else
#endif
        rc = prcnn_train_stack_fwd(&S, L, c.nl, ns, dump, ldd, A(11), nlast, 0, arg, work, (size_t)1 << 62, nullptr);
    fwd = harvest(rc);
    if (rc != PRCNN_OK) return;                                   // (no backward without a forward)
#ifndef TRAIN_SPLIT_RECORD_FP32_ONLY
    if (split) rc = prcnn_train_stack_bwd_split(&S, L, c.nl, ns, dump, ldd, A(13), nlast, arg, gin, ld_gin, wst, work, (size_t)1 << 62, nullptr);
    else
#endif
        rc = prcnn_train_stack_bwd(&S, L, c.nl, ns, dump, ldd, A(13), nlast, arg, gin, ld_gin, work, (size_t)1 << 62, nullptr);
    bwd = harvest(rc);
}

static bool starts(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

static void sweep() {
    static const long ROWS[] = {1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 4096, 6016, 6017, 12160, 12161, 24448, 24449, 100000, 2000000};
    static const int CH[] = {3, 4, 16, 32, 33, 64, 65, 96, 128, 256, 512};
    std::set<std::string> seen;
    for (long rows : ROWS)
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
                                Case c = {source, r, ns, bn, need_x, 3, {K, N, (K + 3) / 4 * 4, N}};
                                for (int nl = 3; nl >= 1; nl -= 2) {
                                    c.nl = nl;
                                    std::vector<Launch> f, b;
                                    run_case(c, true, f, b);
                                    for (const Launch& x : f) seen.insert(x.name);
                                    for (const Launch& x : b) seen.insert(x.name);
                                }
                            }
            }
    for (const std::string& s : seen) printf("%s\n", s.c_str());
}

int main(int argc, char** argv) {
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    prcnn_switch_reload();
    if (argc > 1 && strcmp(argv[1], "--sweep") == 0) {
        sweep();
    } else if (argc >= 9 && (strcmp(argv[1], "--case") == 0 || strcmp(argv[1], "--fp32-case") == 0)) {
        const bool split = strcmp(argv[1], "--case") == 0;
        Case c = {};
        const std::string src = argv[2];
        c.source = src == "plain" ? 0 : src == "group" ? 1 : src == "interp" ? 2 : src == "flat" ? 3 : -1;
        if (c.source < 0) { fprintf(stderr, "unknown source %s\n", argv[2]); return 2; }
        c.rows = atol(argv[3]); c.pool_ns = atoi(argv[4]); c.bn = atoi(argv[5]); c.need_x = atoi(argv[6]);
        c.nl = argc - 8;
        if (c.nl > 8) { fprintf(stderr, "at most 8 layers\n"); return 2; }
        for (int i = 0; i <= c.nl; i++) c.chans[i] = atoi(argv[7 + i]);
        std::vector<Launch> f, b;
        run_case(c, split, f, b);
        if (!split) {
            for (const Launch& x : f) printf("%s %s\n", x.name.c_str(), x.shape.c_str());
            for (const Launch& x : b) printf("%s %s\n", x.name.c_str(), x.shape.c_str());
        } else {
            std::set<std::string> also;
            int l = 0;
            for (const Launch& x : f)
                if (starts(x.name, "train_fwd_")) printf("fwd %d %s\n", l++, x.name.c_str());
                else also.insert(x.name);
            // dgrad follows the layer's wgrad reduction, last layer first; layer 0 has one only when its input takes a gradient
            l = c.nl;
            for (const Launch& x : b) {
                if (starts(x.name, "bn_bwd_reduce_kernel")) l--;
                if (starts(x.name, "train_dgrad_")) printf("dgrad %d %s\n", l, x.name.c_str());
                else also.insert(x.name);
            }
            for (const std::string& s : also) printf("also %s\n", s.c_str());
        }
    } else {
        fprintf(stderr, "usage: train_split_launch_record --sweep | --case|--fp32-case SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]\n");
        return 2;
    }
    return g_failed ? 1 : 0;
}
