// Host driver for csrc/rpn_loss_math.h (tests/test_rpn_loss_math_cpu.py; built once plain and once with -fsanitize=address,undefined).
//   rpn_loss_math_host MODE in.bin out.bin [gamma alpha]      float32 records in, float32 / int32 records out, default configuration
//     labels   7 floats [dx dy dz h w l ry]      -> 3 int32 bins (x, z, ry) + 6 floats (x, z, ry residuals, 3 size targets)
//     focal    3 floats [logit, target, weight]  -> 2 floats (term, d term / d logit)
//     softmax  13 floats [12 logits, target]     -> 13 floats (term, 12 derivatives)
//     sl1      2 floats [a, b]                   -> 2 floats (term, d term / d a)
//     row      C + 7 floats [prediction row, 7 labels] -> 8 + C floats (terms x_bin z_bin x_res z_res y ry_bin ry_res size, then
//              the row's gradient for g = 1); C of the default configuration (76)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rpn_loss_math.h"

int main(int argc, char** argv) {
    if (argc != 4 && argc != 6) return 2;
    const double mean_size[3] = {1.52563191462, 1.62856739989, 3.88311640418};
    const double gamma = argc == 6 ? std::atof(argv[4]) : 2.0;
    const double alpha = argc == 6 ? std::atof(argv[5]) : 0.25;
    const RlConfig c = rl_make_config(3.0, 0.5, 12, 1, mean_size, gamma, alpha, alpha >= 0.0, 1.0, 1.0);
    const char* mode = argv[1];
    int in_w;
    if (!std::strcmp(mode, "labels")) in_w = 7;
    else if (!std::strcmp(mode, "focal")) in_w = 3;
    else if (!std::strcmp(mode, "softmax")) in_w = 13;
    else if (!std::strcmp(mode, "sl1")) in_w = 2;
    else if (!std::strcmp(mode, "row")) in_w = c.C + 7;
    else return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    std::vector<float> rec(in_w), res;
    while (std::fread(rec.data(), sizeof(float), in_w, in) == (size_t)in_w) {
        res.clear();
        if (in_w == 7) {
            int b[3];
            float r[6];
            rl_bin_and_residual(rec[0], c, &b[0], &r[0]);
            rl_bin_and_residual(rec[2], c, &b[1], &r[1]);
            rl_angle_bin_and_residual(rec[6], c, &b[2], &r[2]);
            for (int k = 0; k < 3; ++k) r[3 + k] = rl_size_target(rec[3 + k], c.anchor[k]);
            for (int k = 0; k < 3; ++k) {
                float f;
                const int32_t v = b[k];
                std::memcpy(&f, &v, 4);
                res.push_back(f);
            }
            res.insert(res.end(), r, r + 6);
        } else if (in_w == 3) {
            float v, d;
            rl_focal(rec[0], rec[1], rec[2], c, &v, &d);
            res = {v, d};
        } else if (in_w == 13) {
            float m, ls;
            const int t = (int)rec[12];
            res.push_back(rl_softmax_ce(rec.data(), 12, t, &m, &ls));
            for (int j = 0; j < 12; ++j) res.push_back(rl_softmax_ce_grad(rec[j], m, ls, j == t));
        } else if (in_w == 2) {
            float d;
            const float v = rl_smooth_l1(rec[0], rec[1], &d);
            res = {v, d};
        } else {
            float acc[RL_TERMS] = {0};
            std::vector<float> row(rec.begin(), rec.begin() + c.C);
            rl_reg_row<false, float>(row.data(), rec.data() + c.C, c, 1.0f, acc);
            res.insert(res.end(), acc + RL_X_BIN, acc + RL_TERMS);
            rl_reg_row<true, float>(row.data(), rec.data() + c.C, c, 1.0f, acc);
            res.insert(res.end(), row.begin(), row.end());
        }
        if (std::fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
