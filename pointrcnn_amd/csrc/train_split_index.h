// train_split_index.h -- which weight element a position of a training split image holds (csrc/mlp_train.h:
// train_pack_split_all_kernel), as plain host / device arithmetic so that tests/train_split_index_host.cpp can walk it on the CPU.
//
// An image is [column block][k-step][piece][lane] (pack_weight_split_kernel's chain = 0 layout): "row" r = 32 nb + (lane & 31) is the
// GEMM's output column, k = 16 ks + 8 (lane >> 5) + e its reduction index, KS = 2 ceil(width / 32) k-steps: zero-padded to whole
// 32-wide chunks.  W is (Nout x K), torch layout.
//   forward     row = output channel n, k = the staged row's column.  A grouped first layer stages [features | dxyz] while W's
//               columns are [xyz | features]: column k reads W[n][k + rot] for k < K - rot and W[n][k - (K - rot)] after
//               (rot = 3; train_pack_kernel's rotation of the fp32 image)
//   transposed  (dgrad) row = input channel kin of the `ext` that take a gradient -- a grouped first layer leaves its three xyz
//               columns out (col0 = 3) --, k = output channel n: reads W[n][col0 + kin]
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRAIN_SPLIT_HD __host__ __device__
#else
#define TRAIN_SPLIT_HD
#endif

struct TrainSplitImage {
    int Nout, K;                  // W's shape
    int ext;                      // image rows that exist: Nout (forward), kin_t (transposed)
    int shift;                    // forward: rot; transposed: col0
    int transposed;
    int KS, NB;                   // k-steps (even), column blocks
};

TRAIN_SPLIT_HD static inline TrainSplitImage train_split_image(int Nout, int K, int ext, int shift, int transposed) {
    TrainSplitImage I;
    I.Nout = Nout; I.K = K; I.ext = ext; I.shift = shift; I.transposed = transposed;
    I.KS = (((transposed ? Nout : K) + 31) / 32) * 2;
    I.NB = (ext + 31) / 32;
    return I;
}
// threads (= 16-byte lanes per piece) of one image
TRAIN_SPLIT_HD static inline long train_split_threads(const TrainSplitImage& I) { return (long)I.NB * I.KS * 64; }
TRAIN_SPLIT_HD static inline long train_split_bytes(const TrainSplitImage& I) { return train_split_threads(I) * 3 * 16; }
// index into W of image position (row, k), or -1: padding (+0)
TRAIN_SPLIT_HD static inline long train_split_src(const TrainSplitImage& I, int row, int k) {
    if (row >= I.ext) return -1;
    if (I.transposed) return k < I.Nout ? (long)k * I.K + I.shift + row : -1;
    if (k >= I.K) return -1;
    const int ko = k < I.K - I.shift ? k + I.shift : k - (I.K - I.shift);
    return (long)row * I.K + ko;
}
