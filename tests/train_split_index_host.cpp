// Stand-alone host program: the index arithmetic of train_pack_split_all_kernel (csrc/train_split_index.h) walked on the CPU.
// For (Nout, K, rot) in {(32, 36, 0), (64, 99, 3), (196, 128, 0)}, forward and transposed (a rot = 3 layer leaves its xyz columns out):
//   * every element of W that the GEMM reads is held by exactly one image position, no element twice, none of the others at all;
//   * a forward position (n, k) holds W[n][(k + rot) mod K] (train_pack_kernel's rotation), a transposed one (kin, n) W[n][rot + kin];
//   * every position past the width or past the rows is padding (-1), and the image is whole 32-wide chunks: KS even, KS * 16 >= width;
//   * the thread count covers NB * KS * 64 lanes and the byte size is 48 bytes per lane.
// Built and run by tests/test_train_split_all_cpu.py with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>

#include "train_split_index.h"

static int g_bad = 0;
#define CHECK(c) do { if (!(c)) { g_bad++; fprintf(stderr, "line %d: %s (Nout %d K %d rot %d t %d)\n", __LINE__, #c, Nout, K, rot, t); } } while (0)

int main() {
    static const int SHAPES[3][3] = {{32, 36, 0}, {64, 99, 3}, {196, 128, 0}};
    for (const auto& sh : SHAPES)
        for (int t = 0; t < 2; t++) {
            const int Nout = sh[0], K = sh[1], rot = sh[2];
            const int ext = t ? K - rot : Nout, width = t ? Nout : K;
            const TrainSplitImage I = train_split_image(Nout, K, ext, rot, t);
            CHECK(I.KS % 2 == 0 && I.KS * 16 >= width && I.KS * 16 < width + 32 && I.NB * 32 >= ext && I.NB * 32 < ext + 32);
            CHECK(train_split_threads(I) == (long)I.NB * I.KS * 64 && train_split_bytes(I) == train_split_threads(I) * 48);
            std::vector<int> hits((size_t)Nout * K, 0);
            for (int row = 0; row < I.NB * 32; row++)
                for (int k = 0; k < I.KS * 16; k++) {
                    const long s = train_split_src(I, row, k);
                    if (row >= ext || k >= width) { CHECK(s == -1); continue; }
                    CHECK(s >= 0 && s < (long)Nout * K);
                    if (s < 0 || s >= (long)Nout * K) continue;
                    hits[s]++;
                    if (t) CHECK(s == (long)k * K + rot + row);
                    else CHECK(s == (long)row * K + (k + rot) % K);
                }
            for (int n = 0; n < Nout; n++)
                for (int k = 0; k < K; k++) CHECK(hits[(size_t)n * K + k] == ((t && k < rot) ? 0 : 1));
        }
    printf("%s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
