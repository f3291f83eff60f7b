// Host driver for the adam and sgd updates of csrc/optim_math.h (tests/optim_modes_cases.py run_host; built once plain and once with
// -fsanitize=address,undefined): a list of tensors over several steps, element by element in the header's arithmetic.
//   optim_modes_host in.bin out.bin
//     in   4 int32 [T tensors, S steps, has_coef, mode (1 adam, 2 sgd)], 1 float max_norm (0: no clip), T int64 sizes, T int32 has_grad,
//          the parameters, exp_avg (sgd: the momentum buffer) and exp_avg_sq of all tensors (flat float32, tensor after tensor),
//          per step: 7 floats -- adam [wd, 1 - beta1, beta2, 1 - beta2, sqrt(1 - beta2^t), eps, -(lr / (1 - beta1^t))], sgd [wd, momentum,
//          -lr, 0, 0, 0, 0] --, 1 float coef (used when has_coef), the gradients of all tensors (ignored for a tensor with has_grad 0)
//     out  parameters, exp_avg, exp_avg_sq (flat float32), S floats norm, S floats coef
//   without has_coef the norm is float(sqrt(sum of g^2 in double, in element order)) and coef = om_clip_coef(norm, max_norm).
//   A tensor with has_grad 0 is not touched.  sgd with momentum 0 does not touch the buffer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "optim_math.h"

static bool read_floats(FILE* in, std::vector<float>& v) { return v.empty() || std::fread(v.data(), sizeof(float), v.size(), in) == v.size(); }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) return 3;
    int32_t head[4];
    float max_norm;
    if (std::fread(head, sizeof(int32_t), 4, in) != 4 || std::fread(&max_norm, sizeof(float), 1, in) != 1) return 3;
    const int T = head[0], S = head[1], has_coef = head[2], mode = head[3];
    if (T < 0 || S < 0 || (mode != 1 && mode != 2)) return 2;
    std::vector<int64_t> sizes(T);
    std::vector<int32_t> has_grad(T);
    if (T && (std::fread(sizes.data(), sizeof(int64_t), T, in) != (size_t)T || std::fread(has_grad.data(), sizeof(int32_t), T, in) != (size_t)T))
        return 3;
    size_t total = 0;
    for (int64_t n : sizes) {
        if (n < 0) return 2;
        total += (size_t)n;
    }
    std::vector<float> p(total), m(total), v(total), g(total), norms(S), coefs(S);
    if (!read_floats(in, p) || !read_floats(in, m) || !read_floats(in, v)) return 3;
    for (int s = 0; s < S; ++s) {
        float sc[7], coef;
        if (std::fread(sc, sizeof(float), 7, in) != 7 || std::fread(&coef, sizeof(float), 1, in) != 1 || !read_floats(in, g)) return 3;
        const OmAdamL2 a = {sc[0], sc[1], sc[2], sc[3], sc[4], sc[5], sc[6]};
        const OmSgd q = {sc[0], sc[1], sc[2]};
        double sum = 0.0;
        size_t off = 0;
        for (int t = 0; t < T; ++t) {
            if (has_grad[t])
                for (int64_t i = 0; i < sizes[t]; ++i) sum += (double)g[off + i] * (double)g[off + i];
            off += (size_t)sizes[t];
        }
        const float norm = (float)std::sqrt(sum);
        if (!has_coef) coef = max_norm > 0.0f ? om_clip_coef(norm, max_norm) : 1.0f;
        norms[s] = norm;
        coefs[s] = coef;
        off = 0;
        for (int t = 0; t < T; ++t) {
            for (int64_t i = 0; has_grad[t] && i < sizes[t]; ++i) {
                const size_t j = off + (size_t)i;
                if (mode == 1) om_adam_l2(&p[j], g[j], &m[j], &v[j], coef, a);
                else if (q.momentum != 0.0f) om_sgd(&p[j], g[j], &m[j], coef, q);
                else om_sgd_plain(&p[j], g[j], coef, q);
            }
            off += (size_t)sizes[t];
        }
    }
    auto put = [&](const std::vector<float>& x) { return x.empty() || std::fwrite(x.data(), sizeof(float), x.size(), out) == x.size(); };
    if (!put(p) || !put(m) || !put(v) || !put(norms) || !put(coefs)) return 4;
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 4;
}
