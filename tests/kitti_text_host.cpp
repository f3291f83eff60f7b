// Host driver for csrc/kitti_text_math.h (tests/kitti_text_cases.py; built once plain and once with -fsanitize=address,undefined): what
// csrc/kitti_text.hip computes, frame after frame and candidate after candidate.
//   kitti_text_host fmt in.bin out.bin
//     in   1 int64 n, n float64
//     out  n records of 18 bytes: the length of " %.4f" of the value (255: outside the domain, nothing printed), then 17 bytes, zero padded
//   kitti_text_host lines in.bin out.bin
//     in   5 int32 [B, M, has_keep, has_num, class length], 16 bytes class name, boxes (B,M,7) f32, scores (B,M) f32, keep (B,M) i32,
//          num (B) i32, P2 (B,12) f64, img_hw (B,2) i32 [H, W]   (keep / num are present in the file either way)
//     out  text (B, M*256) u8 (zeros past text_len), text_len (B) i32, status (B) i32, rows (B,M,13) f64, valid (B,M) u8
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "kitti_text_math.h"

template <class T>
static bool get(FILE* in, std::vector<T>& v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), in) == v.size(); }
template <class T>
static bool put(FILE* out, const std::vector<T>& v) { return v.empty() || std::fwrite(v.data(), sizeof(T), v.size(), out) == v.size(); }

static int run_fmt(FILE* in, FILE* out) {
    int64_t n;
    if (std::fread(&n, sizeof n, 1, in) != 1 || n < 0) return 3;
    std::vector<double> x((size_t)n);
    if (!get(in, x)) return 3;
    std::vector<unsigned char> rec((size_t)n * 18, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int len = kt_fixed4(x[(size_t)i], &rec[(size_t)i * 18 + 1]);
        rec[(size_t)i * 18] = len < 0 ? 255 : (unsigned char)len;
    }
    return put(out, rec) ? 0 : 4;
}

static int run_lines(FILE* in, FILE* out) {
    int32_t head[5];
    char name[16];
    if (std::fread(head, sizeof(int32_t), 5, in) != 5 || std::fread(name, 1, 16, in) != 16) return 3;
    const int B = head[0], M = head[1], has_keep = head[2], has_num = head[3], cl = head[4];
    if (B < 0 || M < 0 || cl < 1 || cl > KT_CLASS_MAX) return 2;
    const size_t BM = (size_t)B * (size_t)M;
    std::vector<float> boxes(BM * 7), scores(BM);
    std::vector<int32_t> keep(BM), num((size_t)B), hw((size_t)B * 2);
    std::vector<double> P2((size_t)B * 12);
    if (!get(in, boxes) || !get(in, scores) || !get(in, keep) || !get(in, num) || !get(in, P2) || !get(in, hw)) return 3;
    std::vector<unsigned char> text(BM * KT_LINE_MAX, 0), valid(BM, 0), prefix;
    std::vector<int32_t> text_len((size_t)B, 0), status((size_t)B, 0);
    std::vector<double> rows(BM * KT_FIELDS, 0.0);
    for (int k = 0; k < cl; ++k) prefix.push_back((unsigned char)name[k]);
    for (const char* p = " -1 -1"; *p; ++p) prefix.push_back((unsigned char)*p);
    for (int b = 0; b < B; ++b) {
        int n = has_num ? num[(size_t)b] : M, flag = 0, base = 0;
        if (n < 0 || n > M) {
            flag = 2;
            n = 0;
        }
        unsigned char* out_b = text.data() + (size_t)b * M * KT_LINE_MAX;
        for (int j = 0; j < n; ++j) {
            const int idx = has_keep ? keep[(size_t)b * M + j] : j;
            if (idx < 0 || idx >= M) {
                flag |= 2;
                continue;
            }
            double* row = &rows[((size_t)b * M + j) * KT_FIELDS];
            const int ok = kt_box_row(&boxes[((size_t)b * M + idx) * 7], scores[(size_t)b * M + idx], &P2[(size_t)b * 12], hw[2 * (size_t)b],
                                      hw[2 * (size_t)b + 1], row, 1);
            valid[(size_t)b * M + j] = (unsigned char)ok;
            if (!ok) continue;
            unsigned char line[KT_LINE_MAX];
            const int len = kt_line(row, 1, prefix.data(), (int)prefix.size(), line);
            if (len < 0) {
                flag |= 1;
                continue;
            }
            std::memcpy(out_b + base, line, (size_t)len);
            base += len;
        }
        status[(size_t)b] = (flag & 2) ? 2 : (flag & 1);
        text_len[(size_t)b] = flag ? 0 : base;
        if (flag) std::memset(out_b, 0, (size_t)M * KT_LINE_MAX);
    }
    return put(out, text) && put(out, text_len) && put(out, status) && put(out, rows) && put(out, valid) ? 0 : 4;
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* in = std::fopen(argv[2], "rb");
    FILE* out = std::fopen(argv[3], "wb");
    if (!in || !out) return 3;
    int rc = 2;
    if (std::strcmp(argv[1], "fmt") == 0) rc = run_fmt(in, out);
    else if (std::strcmp(argv[1], "lines") == 0) rc = run_lines(in, out);
    std::fclose(in);
    if (std::fclose(out) != 0 && rc == 0) rc = 4;
    return rc;
}
