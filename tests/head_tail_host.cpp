// Host driver for csrc/head_tail_math.h (tests/test_head_tail_cpu.py): the Dropout mask of the training heads' tail, entry by entry.
//   head_tail_host seed stream call R K p out.bin
//     out  R * K bytes, keep(seed, stream, call, r, k) in row-major order, then one float32: head_tail_scale(p)
//   p is parsed as a double and rounded to float32 once, as the Python twin does.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "head_tail_math.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const unsigned seed = (unsigned)std::strtoul(argv[1], nullptr, 10), stream = (unsigned)std::strtoul(argv[2], nullptr, 10);
    const unsigned call = (unsigned)std::strtoul(argv[3], nullptr, 10);
    const long R = std::strtol(argv[4], nullptr, 10), K = std::strtol(argv[5], nullptr, 10);
    const float p = (float)std::strtod(argv[6], nullptr);
    if (R < 1 || K < 1 || !(p >= 0.0f && p < 1.0f)) return 2;
    std::vector<uint8_t> keep((size_t)R * (size_t)K);
    const unsigned key = head_tail_key(seed, stream, call);
    for (long r = 0; r < R; ++r)
        for (long k = 0; k < K; ++k) {
            const bool a = head_tail_keep(seed, stream, call, (unsigned long long)r, (unsigned)K, (unsigned)k, p);
            const bool b = head_tail_keep_i(key, (unsigned)((unsigned long long)r * (unsigned long long)K + (unsigned long long)k), p);
            if (a != b) return 4;                    // the kernels' hoisted key and the definition are the same function
            keep[(size_t)r * (size_t)K + (size_t)k] = a ? 1 : 0;
        }
    const float scale = head_tail_scale(p);
    if (head_tail_drop(3.0f, false, scale) != 0.0f || head_tail_drop(3.0f, true, scale) != 3.0f * scale) return 4;
    FILE* out = std::fopen(argv[7], "wb");
    if (!out) return 3;
    const bool ok = std::fwrite(keep.data(), 1, keep.size(), out) == keep.size() && std::fwrite(&scale, sizeof(float), 1, out) == 1;
    return std::fclose(out) == 0 && ok ? 0 : 3;
}
