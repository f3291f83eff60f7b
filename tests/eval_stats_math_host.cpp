// Host driver for csrc/eval_stats_math.h (tests/test_eval_stats_math_cpu.py; built once plain and once with -fsanitize=address,undefined).
//   eval_stats_math_host thresh in.bin out.bin        float32 values in -> per value 5 floats, 1 where es_recalled(v, t) at 0.1 0.3 0.5 0.7 0.9
//   eval_stats_math_host accumulate in.bin out.bin    batches in, es_accumulate_serial over all of them -> one EsState (160 bytes)
//   eval_stats_math_host each in.bin out.bin          the same with a zeroed state per batch -> one EsState per batch
// A batch: int32 header [S B G has_det N label_is_i64 seg_mode R], float32 [cls_fg cls_bg refine_thresh], then gt_max (S*B*G f32),
// num_gt (B i32), det_num (B i32, has_det), seg (B*N f32) and labels (B*N i32 | i64) when N > 0, pred_class (B*R u8) and gt_iou (B*R f32)
// when R > 0.  Every array is read into a buffer of exactly its size.
#include <cstdio>
#include <cstring>
#include <vector>
#include "eval_stats_math.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    if (!std::strcmp(argv[1], "thresh")) {
        float v;
        while (std::fread(&v, sizeof(float), 1, in) == 1) {
            float r[ES_THRESHOLDS];
            for (int t = 0; t < ES_THRESHOLDS; ++t) r[t] = es_recalled(v, t) ? 1.0f : 0.0f;
            if (std::fwrite(r, sizeof(float), ES_THRESHOLDS, out) != (size_t)ES_THRESHOLDS) return 4;
        }
    } else {
        const bool each = !std::strcmp(argv[1], "each");
        if (!each && std::strcmp(argv[1], "accumulate")) return 2;
        EsState st;
        std::memset(&st, 0, sizeof st);
        int32_t h[8];
        bool any = false;
        while (std::fread(h, sizeof(int32_t), 8, in) == 8) {
            float thr[3];
            if (std::fread(thr, sizeof(float), 3, in) != 3) return 5;
            const size_t S = h[0], B = h[1], G = h[2], N = h[4], R = h[7];
            std::vector<float> gt_max, seg, gt_iou;
            std::vector<int32_t> num_gt, det, lab32;
            std::vector<int64_t> lab64;
            std::vector<uint8_t> pred;
            if (!read_n(in, gt_max, S * B * G) || !read_n(in, num_gt, B) || !read_n(in, det, h[3] ? B : 0) || !read_n(in, seg, B * N)) return 5;
            if (!(h[5] ? read_n(in, lab64, B * N) : read_n(in, lab32, B * N))) return 5;
            if (!read_n(in, pred, B * R) || !read_n(in, gt_iou, B * R)) return 5;
            EsBatch P;
            P.gt_max = gt_max.data(); P.num_gt = num_gt.data(); P.S = (int)S; P.B = (int)B; P.G = (int)G;
            P.det_num = h[3] ? det.data() : nullptr;
            P.seg = N ? seg.data() : nullptr;
            P.cls_label = !N ? nullptr : h[5] ? (const void*)lab64.data() : (const void*)lab32.data();
            P.label_is_i64 = h[5]; P.seg_mode = h[6]; P.N = (int64_t)N;
            P.pred_class = R ? pred.data() : nullptr; P.gt_iou = R ? gt_iou.data() : nullptr; P.R = (int)R;
            P.cls_fg = thr[0]; P.cls_bg = thr[1]; P.refine_thresh = thr[2];
            if (each) std::memset(&st, 0, sizeof st);
            es_accumulate_serial(P, &st);
            any = true;
            if (each && std::fwrite(&st, sizeof st, 1, out) != 1) return 4;
        }
        if (!each && any && std::fwrite(&st, sizeof st, 1, out) != 1) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
