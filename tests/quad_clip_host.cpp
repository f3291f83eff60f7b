// Host driver for csrc/quad_clip.h (tests/test_quad_exact_cpu.py): reads pairs of (8,3) fp32 corner sets, 48 floats per pair,
// from argv[1]; writes iou3d and iou_bev, 2 floats per pair, to argv[2].  The steps are corner_iou3d_kernel's (csrc/train_input.hip).
#include <cmath>
#include <cstdio>
#include <vector>
#include "quad_clip.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    float c[48];
    std::vector<float> res;
    while (std::fread(c, sizeof(float), 48, in) == 48) {
        float lo_a, hi_a, lo_b, hi_b, v3 = 0.0f, vb = 0.0f;
        qc_heights(c, lo_a, hi_a);
        qc_heights(c + 24, lo_b, hi_b);
        const float h = qc_h_overlap(lo_a, hi_a, lo_b, hi_b);
        if (h != 0.0f) {
            const QcQuad qa = qc_make(c), qb = qc_make(c + 24);
            qc_ratios(qa, qb, h, hi_a - lo_a, hi_b - lo_b, v3, vb);
        }
        res.push_back(v3);
        res.push_back(vb);
    }
    const bool ok = std::fwrite(res.data(), sizeof(float), res.size(), out) == res.size();
    std::fclose(in);
    return std::fclose(out) == 0 && ok ? 0 : 4;
}
