// Host driver for csrc/rcnn_offline_math.h (tests/test_rcnn_offline_cpu.py; built once plain and once with -fsanitize=address,undefined).
//   rcnn_offline_math_host MODE in.bin out.bin      records of 4-byte words in, records of 4-byte words out
//     iou    14 floats [box a, box b]                                         -> 1 float: get_iou3d on the float32 corners of both (several-box form)
//     slot   14 floats [sampled RoI, its label] + 5 int32 [times, method, seed, frame, slot]
//                                                                             -> 7 floats (the slot's RoI), 1 float (its IoU), 1 int32 (attempts)
//     finish 17 floats [RoI after the noise loop, its label, one pooled point] + 4 int32 [method mask, seed, frame, slot]
//                                                                             -> 7 + 7 + 7 floats (augmented RoI, label, gt_boxes3d_ct), 3 floats (the point)
//   the noise loop's threshold is min(REG_FG_THRESH, CLS_FG_THRESH) = 0.55; AUG_METHOD_PROB[2] = 0.5, AUG_ROT_RANGE = 18
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "rcnn_offline_math.h"

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const bool slot = !std::strcmp(argv[1], "slot");
    const bool finish = !std::strcmp(argv[1], "finish");
    if (!slot && !finish && std::strcmp(argv[1], "iou")) return 2;
    const size_t in_w = slot ? 19 : finish ? 21 : 14;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    std::vector<float> rec(in_w), res;
    while (std::fread(rec.data(), sizeof(float), in_w, in) == in_w) {
        res.clear();
        if (finish) {
            int32_t a[4];
            std::memcpy(a, rec.data() + 17, sizeof(a));
            if (a[0] < 0 || a[0] > 7) return 2;
            const RoAug g = ro_aug_draw((unsigned)a[1], (unsigned)a[2], (unsigned)a[3], a[0], 0.5, 18.0);
            float roi[7], gt[7], ct[7], p[3] = {rec[14], rec[15], rec[16]};
            std::memcpy(roi, rec.data(), sizeof(roi));
            std::memcpy(gt, rec.data() + 7, sizeof(gt));
            const RoCanon cn = ro_finish_boxes(roi, gt, g, ct);
            ro_aug_point(p, g);
            ro_canon_point(p, cn);
            res.insert(res.end(), roi, roi + 7);
            res.insert(res.end(), gt, gt + 7);
            res.insert(res.end(), ct, ct + 7);
            res.insert(res.end(), p, p + 3);
            if (std::fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) return 4;
            continue;
        }
        float cb[24];
        ro_corners_f32(rec.data() + 7, cb, slot);
        if (!slot) {
            float ca[24];
            ro_corners_f32(rec.data(), ca, false);
            res.push_back(ro_pair_iou(ca, cb));
        } else {
            int32_t a[5];
            std::memcpy(a, rec.data() + 14, sizeof(a));
            if (a[0] < 0 || a[0] > RO_MAX_AUG_TIMES || (a[1] != 0 && a[1] != 1)) return 2;
            float roi[7], iou, f;
            const int32_t cnt = ro_noise_slot(rec.data(), cb, a[0], 0.55, (unsigned)a[2], (unsigned)a[3], (unsigned)a[4], a[1], roi, &iou);
            res.insert(res.end(), roi, roi + 7);
            res.push_back(iou);
            std::memcpy(&f, &cnt, 4);
            res.push_back(f);
        }
        if (std::fwrite(res.data(), sizeof(float), res.size(), out) != res.size()) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
