// Host driver for csrc/roi_sample.h (tests/test_roi_sample_cpu.py; built once plain and once with -fsanitize=address,undefined): phase 2
// of both RoI samplers, in the order the kernels run it -- clear, lists, the caller's tail, plan, the caller's foreground-only action,
// keys, ranks, background picks -- with everything the two kernels do differently as an input.
//   roi_sample_host in.bin out.bin      one record of 4-byte words per frame in, one per frame out
//     in   12 int32 [n, ntail, R, ng, seed, frame, key_by_roi, fg_only_fills, stream_key, stream_replace, stream_hard, stream_easy]
//              n            row maxima; ntail  entries appended to the foreground list after the scan (the offline labels' best RoIs)
//              ng           live ground-truth boxes: 0 = the kernels' status 2, nothing is sampled
//              key_by_roi   1: the key of place t is r(stream_key, frame, fg[t]) (online), 0: r(stream_key, frame, t) (offline)
//              fg_only_fills  what a frame with foreground but no background candidate gets: 1 = all R slots, drawn with
//                           replacement from stream_replace (online), 0 = status 1 (offline)
//          6 doubles cfg6 (REG_FG, CLS_FG, CLS_BG, CLS_BG_LO, FG_RATIO, HARD_BG_RATIO), n floats, ntail int32
//     out  9 + R int32 [nfg, nhard, neasy, fs, status, kind, fs, bs, nh, src[R]]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "roi_sample.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t h[12];
    while (std::fread(h, sizeof(int32_t), 12, in) == 12) {
        const int n = h[0], ntail = h[1], R = h[2], ng = h[3];
        const unsigned seed = (unsigned)h[4], frame = (unsigned)h[5];
        if (n < 0 || ntail < 0 || R <= 0) return 2;
        double cfg6[6];
        std::vector<float> mo(n), box(2 * 7 * (size_t)R + R);
        std::vector<int32_t> tail(ntail), res(9 + (size_t)R, 0);
        if (std::fread(cfg6, sizeof(double), 6, in) != 6 || std::fread(mo.data(), sizeof(float), n, in) != (size_t)n ||
            std::fread(tail.data(), sizeof(int32_t), ntail, in) != (size_t)ntail) return 3;
        const RsCfg c = rs_cfg(cfg6, R);
        std::vector<int> fg(n + ntail), hard(n), easy(n);
        std::vector<unsigned> keys(n + ntail);
        int32_t* src = res.data() + 9;
        for (int tid = 0; tid < 3; ++tid) rs_clear(box.data(), box.data() + 7 * (size_t)R, box.data() + 14 * (size_t)R, src, R, tid, 3);
        for (float v : box)
            if (v != 0.f) return 5;
        if (ng > 0) {
            RsLists l = rs_lists(mo.data(), n, c, fg.data(), hard.data(), easy.data());
            for (int j = 0; j < ntail; ++j) fg[l.nfg++] = tail[j];
            RsPlan p = rs_plan(l, R, c.fg_per_image, c.hard_ratio);
            const int kind = p.kind;
            if (p.kind == RS_FG_ONLY && h[7]) {
                p.fs = R;
                for (int t = 0; t < R; ++t) src[t] = fg[rs_below(scene_rand(seed, (unsigned)h[9], frame, (unsigned)t), l.nfg)];
            }
            if (p.kind == RS_BOTH) {
                for (int t = 0; t < l.nfg; ++t) keys[t] = scene_rand(seed, (unsigned)h[8], frame, h[6] ? (unsigned)fg[t] : (unsigned)t);
                for (int t = 0; t < l.nfg; ++t) {
                    const int rank = rs_rank(keys.data(), l.nfg, t);
                    if (rank < p.fs) src[rank] = fg[t];
                }
            }
            for (int t = 0; t < p.bs; ++t) src[p.fs + t] = rs_bg_pick(t, p, l, hard.data(), easy.data(), seed, (unsigned)h[10], (unsigned)h[11], frame);
            const int32_t head[9] = {l.nfg, l.nhard, l.neasy, p.fs, p.fs + p.bs == 0 ? 1 : 0, kind, p.fs, p.bs, p.nh};
            std::memcpy(res.data(), head, sizeof(head));
        } else {
            res[4] = 2;
        }
        if (std::fwrite(res.data(), sizeof(int32_t), res.size(), out) != res.size()) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
