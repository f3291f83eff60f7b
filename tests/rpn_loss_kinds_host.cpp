// Host driver for the DiceLoss / BinaryCrossEntropy row functions of csrc/rpn_loss_math.h (tests/test_rpn_loss_kinds_cpu.py; built
// once plain and once with -fsanitize=address,undefined).
//   rpn_loss_kinds_host MODE in.bin out.bin      float32 records in, float32 records out
//     bce       3 floats [logit, label, fg_weight]   -> 2 floats (the row's term, d term / d logit)
//     dice      2 floats [logit, label]              -> 4 floats (min(p, t), max(p, t) and their derivatives in the logit)
//     dicegrad  5 floats [logit, label, A, B, k]     -> 1 float  (d loss / d logit with the sums A, B and the factor k)
//   label is -1 (ignored), 0 or 1, as rl_label folds it
#include <cstdio>
#include <cstring>
#include <vector>
#include "rpn_loss_math.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const char* mode = argv[1];
    int in_w;
    if (!std::strcmp(mode, "bce")) in_w = 3;
    else if (!std::strcmp(mode, "dice")) in_w = 2;
    else if (!std::strcmp(mode, "dicegrad")) in_w = 5;
    else return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    std::vector<float> rec(in_w), res;
    while (std::fread(rec.data(), sizeof(float), in_w, in) == (size_t)in_w) {
        const int label = (int)rec[1];
        res.clear();
        if (in_w == 3) {
            float v, d;
            rl_bce_row(rec[0], label, rec[2], &v, &d);
            res = {v, d};
        } else {
            float lo, hi, dlo, dhi;
            rl_dice_row(rec[0], label, &lo, &hi, &dlo, &dhi);
            if (in_w == 2) res = {lo, hi, dlo, dhi};
            else res = {rl_dice_grad(dlo, dhi, (double)rec[2], (double)rec[3], (double)rec[4])};
        }
        if (std::fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
