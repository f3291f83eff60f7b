// Host driver for csrc/aug_scene_math.h (tests/test_aug_scene_cpu.py; built once plain and once with -fsanitize=address,undefined): the
// per-try arithmetic of the offline GT-augmented scene sampler -- the two draws, the range check, the plane move, the enlargement and
// the accept decision on a given IoU -- run against a table the numpy twin (tests/aug_scene_twin.py host_table) writes.
//   aug_scene_host in.bin out.bin
//     in   4 int32 [seed, nframes, D, nboxes], 6 doubles scope, nframes int32 frame ids, then per box 7 floats, 4 doubles plane, 1 float iou
//     out  int32 words: per frame extra_gt_num and the AUGS_TRIES index draws; per box in_scope, the bits of the new y, the bits of the
//          move (2 words), the bits of the enlarged w and l, collides
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "aug_scene_math.h"

static bool put(FILE* out, const void* p, size_t n) { return std::fwrite(p, 1, n, out) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t h[4];
    double scope[6];
    if (std::fread(h, sizeof(int32_t), 4, in) != 4 || std::fread(scope, sizeof(double), 6, in) != 6) return 3;
    const unsigned seed = (unsigned)h[0];
    const int nframes = h[1], D = h[2], nboxes = h[3];
    if (nframes < 0 || nboxes < 0 || D < 2) return 2;
    std::vector<int32_t> frames(nframes);
    if (std::fread(frames.data(), sizeof(int32_t), nframes, in) != (size_t)nframes) return 3;
    for (int f = 0; f < nframes; ++f) {
        std::vector<int32_t> w(1 + AUGS_TRIES);
        w[0] = augs_extra_num(seed, (unsigned)frames[f]);
        for (int t = 0; t < AUGS_TRIES; ++t) w[1 + t] = augs_draw_index(seed, (unsigned)frames[f], t, D);
        if (!put(out, w.data(), w.size() * sizeof(int32_t))) return 4;
    }
    for (int k = 0; k < nboxes; ++k) {
        float box[7], iou, enl[7];
        double plane[4], move;
        if (std::fread(box, sizeof(float), 7, in) != 7 || std::fread(plane, sizeof(double), 4, in) != 4 || std::fread(&iou, sizeof(float), 1, in) != 1)
            return 3;
        int32_t w[7];
        w[0] = augs_in_scope(box, scope) ? 1 : 0;
        const float ny = augs_plane_move(box, plane, move);
        if (augs_point_y(box[1], move) != ny && ny == ny) return 5;      // a point at the box's y moves with it
        augs_enlarge(box, enl);
        std::memcpy(&w[1], &ny, 4);
        std::memcpy(&w[2], &move, 8);
        std::memcpy(&w[4], &enl[4], 4);
        std::memcpy(&w[5], &enl[5], 4);
        w[6] = augs_collides(iou) ? 1 : 0;
        for (int q = 0; q < 7; ++q)
            if (q != 4 && q != 5 && std::memcmp(&enl[q], &box[q], 4) != 0) return 5;
        if (!put(out, w, sizeof(w))) return 4;
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
