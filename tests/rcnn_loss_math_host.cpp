// Host driver for csrc/rcnn_loss_math.h (tests/test_rcnn_loss_math_cpu.py; built once plain and once with -fsanitize=address,undefined).
//   rcnn_loss_math_host MODE in.bin out.bin Y_BY_BIN SIZE_ON_ROI      float32 records in, float32 / int32 records out; the RCNN
//   section's default bins (scope 1.5 / 0.5, y scope 0.5 / 0.25, 9 angle bins), the size anchor the record's or MEAN_SIZE
//     labels   10 floats [dx dy dz h w l ry, 3 anchor sizes] -> 4 int32 bins (x, z, y, ry) + 7 floats (x, z, y, ry residuals, 3 size targets)
//     bce      2 floats [logit, target]                  -> 2 floats (term, d term / d logit)
//     row      C + 10 floats [prediction row, 7 labels, 3 anchor sizes] -> 9 + C floats (terms x_bin z_bin x_res z_res y(offset | bin)
//              y_res ry_bin ry_res size, then the row's gradient for g = 1); C = 46, or 53 with Y_BY_BIN
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "rcnn_loss_math.h"

int main(int argc, char** argv) {
    if (argc != 6) return 2;
    const double mean_size[3] = {1.52563191462, 1.62856739989, 3.88311640418};
    const int y_by_bin = std::atoi(argv[4]), size_on_roi = std::atoi(argv[5]);
    const RcConfig c = rc_make_config(1.5, 0.5, 9, y_by_bin, 0.5, 0.25, size_on_roi, mean_size, RC_LOSS_BCE, 2.0, 0.25, 1);
    const char* mode = argv[1];
    int in_w;
    if (!std::strcmp(mode, "labels")) in_w = 10;
    else if (!std::strcmp(mode, "bce")) in_w = 2;
    else if (!std::strcmp(mode, "row")) in_w = c.C + 10;
    else return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    std::vector<float> rec(in_w), res;
    while (std::fread(rec.data(), sizeof(float), in_w, in) == (size_t)in_w) {
        res.clear();
        const float* anchor = size_on_roi ? rec.data() + in_w - 3 : c.xz.anchor;
        if (in_w == 10) {
            int b[4];
            float r[7];
            rl_bin_and_residual(rec[0], c.xz, &b[0], &r[0]);
            rl_bin_and_residual(rec[2], c.xz, &b[1], &r[1]);
            rl_bin_and_residual(rec[1], c.y, &b[2], &r[2]);
            rc_fine_angle_bin_and_residual(rec[6], c, &b[3], &r[3]);
            for (int k = 0; k < 3; ++k) r[4 + k] = rl_size_target(rec[3 + k], anchor[k]);
            for (int k = 0; k < 4; ++k) {
                float f;
                const int32_t v = b[k];
                std::memcpy(&f, &v, 4);
                res.push_back(f);
            }
            res.insert(res.end(), r, r + 7);
        } else if (in_w == 2) {
            float v, d;
            rc_bce(rec[0], rec[1], &v, &d);
            res = {v, d};
        } else {
            float acc[RC_TERMS] = {0};
            std::vector<float> row(rec.begin(), rec.begin() + c.C);
            rc_reg_row<false, float>(row.data(), rec.data() + c.C, anchor, c, 1.0f, acc);
            res.insert(res.end(), acc + RC_X_BIN, acc + RC_TERMS);
            rc_reg_row<true, float>(row.data(), rec.data() + c.C, anchor, c, 1.0f, acc);
            res.insert(res.end(), row.begin(), row.end());
        }
        if (std::fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
