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
#include "train_record_common.h"

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
                                    run_stack(c, VIA_SPLIT, f, b);
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
        Case c;
        if (!parse_case(argc, argv, 2, 0, c)) return 2;
        std::vector<Launch> f, b;
        run_stack(c, split ? VIA_SPLIT : VIA_FP32, f, b);
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
