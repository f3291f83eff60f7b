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
#include "train_record_common.h"

// the kernels of the backward pass, in order
static std::vector<std::string> run_case(const Case& c, int via) {
    std::vector<Launch> fwd, bwd;
    run_stack(c, via, fwd, bwd);
    std::vector<std::string> out;
    for (const Launch& x : bwd) out.push_back(x.name);
    return out;
}

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
        Case c;
        if (!parse_case(argc, argv, 3, 0, c)) return 2;
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
