// Stand-alone host program: which kernel instantiations the training SharedMLP launches through prcnn_train_stack_fwd_split_all /
// _bwd_split_all (csrc/mlp_train.h) -- recorded, not launched (tests/launch_record_prelude.h), as tests/train_split_launch_record.cpp
// does for the two older split entry points.  The pointers are dummies, never dereferenced; every layer is offered a split image for
// its forward and its dgrad, so the library's own eligibility rules decide.
// Built and run by tests/test_train_split_all_cpu.py (once plain, once with -fsanitize=address,undefined).
//   train_split_all_launch_record --case WG SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]
//                                  one stack through the two new entry points (WG: the wgrad_split flag, 0 / 1):
//                                  "fwd <layer> <kernel> <grid.y>" per forward GEMM in layer order, "dgrad <layer> <kernel> <grid.y>" per
//                                  dgrad GEMM, "packs <forward call> <backward call>" = launches of train_pack_split_all_kernel,
//                                  "also <kernel>" for every other distinct launch
//   train_split_all_launch_record --old-case VIA SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...]
//                                  the same stack through the five older exports (VIA: fp32, split, wsplit): every distinct kernel
//   train_split_all_launch_record --sweep     every distinct kernel of a broad sweep through the new entry points, both WG values
#include "train_record_common.h"

static int call_fwd_all(const Stack& s) {
    return prcnn_train_stack_fwd_split_all(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.out, s.ld_out, s.col_off, s.arg, s.ws, s.work, s.work_bytes, nullptr);
}
static int call_bwd_all(const Stack& s, int wg) {
    return prcnn_train_stack_bwd_split_all(&s.S, s.L, s.nl, s.ns, s.dump, s.ldd, s.gout, s.ld_gout, s.arg, s.gin, s.ld_gin, s.wst, s.work, s.work_bytes,
                                           nullptr, wg);
}
static void run_all(const Case& c, int wg, std::vector<Launch>& fwd, std::vector<Launch>& bwd) {
    Stack s;
    build_stack(c, s);
    const int rc = call_fwd_all(s);
    fwd = harvest(rc);
    bwd.clear();
    if (rc == PRCNN_OK) bwd = harvest(call_bwd_all(s, wg));
}
// "grid x,y,z block ..." -> y
static int grid_y(const std::string& shape) {
    unsigned x = 0, y = 0;
    sscanf(shape.c_str(), "grid %u,%u", &x, &y);
    return (int)y;
}

static void sweep() {
    static const long ROWS[] = {1, 64, 129, 4096, 6016, 6017, 24449, 2000000};
    static const int CH[] = {3, 16, 19, 28, 32, 33, 35, 36, 61, 64, 68, 100, 132, 196, 512, 515};
    std::set<std::string> seen;
    for (long rows : ROWS)
        for (int K : CH)
            for (int N : CH) {
                if (N % 4) continue;                              // (an output width must be a multiple of 4)
                for (int source = 0; source < 4; source++)
                    for (int pool = 0; pool < 2; pool++)
                        for (int need_x = 0; need_x < 2; need_x++) {
                            if ((source == 1 || source == 3) && K < 3) continue;
                            if (source == 3 && !pool) continue;   // padding-free rows are always pooled
                            const int ns = pool ? 16 : 0;
                            const long r = pool ? rows / 16 * 16 : rows;
                            if (r == 0) continue;
                            Case c = {source, r, ns, 1, need_x, 3, {K, N, (K + 3) / 4 * 4, N}};
                            for (int nl = 3; nl >= 1; nl -= 2) {
                                c.nl = nl;
                                for (int wg = 0; wg < 2; wg++) {
                                    std::vector<Launch> f, b;
                                    run_all(c, wg, f, b);
                                    for (const Launch& x : f) seen.insert(x.name);
                                    for (const Launch& x : b) seen.insert(x.name);
                                }
                            }
                        }
            }
    for (const std::string& s : seen) printf("%s\n", s.c_str());
}

int main(int argc, char** argv) {
    for (int i = 0; i < SW_COUNT; i++) unsetenv(prcnn_switch_names[i]);
    prcnn_switch_reload();
    if (argc == 2 && strcmp(argv[1], "--sweep") == 0) {
        sweep();
    } else if (argc >= 10 && strcmp(argv[1], "--case") == 0) {
        Case c;
        if (!parse_case(argc, argv, 3, 0, c)) return 2;
        std::vector<Launch> f, b;
        run_all(c, atoi(argv[2]), f, b);
        std::set<std::string> also;
        int packs_f = 0, packs_b = 0, l = 0;
        for (const Launch& x : f) {
            if (starts(x.name, "train_fwd_")) printf("fwd %d %s %d\n", l++, x.name.c_str(), grid_y(x.shape));
            else if (starts(x.name, "train_pack_split_all_kernel")) packs_f++;
            else also.insert(x.name);
        }
        // dgrad follows the layer's wgrad reduction, last layer first; layer 0 has one only when its input takes a gradient
        l = c.nl;
        for (const Launch& x : b) {
            if (starts(x.name, "bn_bwd_reduce_kernel")) l--;
            if (starts(x.name, "train_dgrad_")) printf("dgrad %d %s %d\n", l, x.name.c_str(), grid_y(x.shape));
            else if (starts(x.name, "train_pack_split_all_kernel")) packs_b++;
            else also.insert(x.name);
        }
        printf("packs %d %d\n", packs_f, packs_b);
        for (const std::string& s : also) printf("also %s\n", s.c_str());
    } else if (argc >= 10 && strcmp(argv[1], "--old-case") == 0) {
        const int via = strcmp(argv[2], "fp32") == 0 ? VIA_FP32 : strcmp(argv[2], "split") == 0 ? VIA_SPLIT : strcmp(argv[2], "wsplit") == 0 ? VIA_WSPLIT : -1;
        Case c;
        if (via < 0 || !parse_case(argc, argv, 3, 0, c)) return 2;
        std::vector<Launch> f, b;
        run_stack(c, via, f, b);
        std::set<std::string> seen;
        for (const Launch& x : f) seen.insert(x.name);
        for (const Launch& x : b) seen.insert(x.name);
        for (const std::string& s : seen) printf("%s\n", s.c_str());
    } else {
        fprintf(stderr, "usage: train_split_all_launch_record --sweep | --case WG SOURCE ROWS POOL_NS BN NEED_X K0 N1 [N2 ...] | --old-case VIA ...\n");
        return 2;
    }
    return g_failed ? 1 : 0;
}
