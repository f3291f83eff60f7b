// kitti_text.hip -- the KITTI result files' text, formatted on the device for a whole batch in one launch (per-box arithmetic and the
// "%.4f" conversion: kitti_text_math.h; host side: pointrcnn_amd/kitti_output.py DeviceResultWriter).
//
// One workgroup of KT_THREADS lanes per frame, candidates in slices of KT_THREADS.  Per slice: lane t takes candidate j = slice + t,
// computes its 13 values into LDS (value-major, so the formatter's loop over the fields indexes LDS, not a private array), runs the
// size test and writes the line's bytes into its own LDS slot (KT_SLOT bytes apart: 65 dwords, the lanes of a wave on different
// banks).  The line lengths are prefix-summed in candidate order (wave scan, then across the waves), and each wave copies whole lines
// from LDS to the frame's text at their packed offsets, 64 consecutive bytes per store.  The running offset carries over the slices,
// so M = 512 takes four of them and nothing but the output is touched in global memory.
//
// A kept box with a field outside the formatter's domain marks the frame status 1; a keep index outside [0, M) or a num outside
// [0, M] marks it status 2 (nothing is read through such an index).  Either way text_len is 0: bytes already copied for the frame mean
// nothing.  rows / valid are written for every j < M (zeros past num).
#include "common.h"
#include "kitti_text_math.h"

constexpr int KT_THREADS = 128;
constexpr int KT_WAVES = KT_THREADS / 64;
constexpr int KT_SLOT = 260;

static_assert(KT_LINE_MAX == PRCNN_KITTI_LINE_MAX, "include/prcnn_pointops.h and kitti_text_math.h disagree on the line bound");
static_assert(KT_CLASS_MAX + 6 + KT_FIELDS * 17 + 1 <= KT_SLOT && KT_SLOT <= KT_LINE_MAX + 4, "a line fits its LDS slot");

struct KtClass {
    uint32_t w[4];      // the class name's bytes, little endian, zero padded
    int len;
};

__global__ __launch_bounds__(KT_THREADS) void kitti_text_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                                const int32_t* __restrict__ keep, const int32_t* __restrict__ num, int M,
                                                                const double* __restrict__ P2, const int32_t* __restrict__ img_hw,
                                                                const KtClass cls, unsigned char* __restrict__ text,
                                                                int32_t* __restrict__ text_len, int32_t* __restrict__ status,
                                                                double* __restrict__ rows, unsigned char* __restrict__ valid) {
    __shared__ double s_row[KT_FIELDS * KT_THREADS];
    __shared__ unsigned char s_line[KT_THREADS * KT_SLOT];
    __shared__ unsigned char s_pre[KT_CLASS_MAX + 6 + 3];
    __shared__ int s_len[KT_THREADS], s_off[KT_THREADS], s_wsum[KT_WAVES], s_flag;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pre_len = cls.len + 6;
    if (tid < KT_CLASS_MAX + 6) {
        const uint32_t word = tid < 4 ? cls.w[0] : (tid < 8 ? cls.w[1] : (tid < 12 ? cls.w[2] : cls.w[3]));
        const int k = tid - cls.len;                                  // " -1 -1" after the name
        const unsigned char tail = (k == 0 || k == 3) ? ' ' : ((k == 1 || k == 4) ? '-' : '1');
        s_pre[tid] = tid < cls.len ? (unsigned char)((word >> (8 * (tid & 3))) & 0xffu) : tail;
    }
    if (tid == 0) s_flag = 0;
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = P2[(size_t)b * 12 + k];
    const int H = img_hw[2 * b], W = img_hw[2 * b + 1];
    int n = num != nullptr ? num[b] : M;
    int flag = 0;
    if (n < 0 || n > M) {
        flag = 2;
        n = 0;
    }
    const int lim = (rows != nullptr || valid != nullptr) ? M : n;
    unsigned char* out = text + (size_t)b * (size_t)M * KT_LINE_MAX;
    unsigned char* my_line = s_line + tid * KT_SLOT;
    int base = 0;
    __syncthreads();
    for (int s0 = 0; s0 < lim; s0 += KT_THREADS) {
        const int j = s0 + tid;
        int len = 0, ok = 0, have = 0;
        if (j < n) {
            const int idx = keep != nullptr ? keep[(size_t)b * M + j] : j;
            if (idx < 0 || idx >= M) {
                flag |= 2;
            } else {
                have = 1;
                const float* bx = boxes + ((size_t)b * M + idx) * 7;
                float box[7];
#pragma unroll
                for (int k = 0; k < 7; ++k) box[k] = bx[k];
                ok = kt_box_row(box, scores[(size_t)b * M + idx], P, H, W, s_row + tid, KT_THREADS);
                if (ok) {
                    len = kt_line(s_row + tid, KT_THREADS, s_pre, pre_len, my_line);
                    if (len < 0) {
                        flag |= 1;
                        len = 0;
                    }
                }
            }
        }
        if (j < M) {
            if (rows != nullptr) {
                double* r = rows + ((size_t)b * M + j) * KT_FIELDS;
                for (int k = 0; k < KT_FIELDS; ++k) r[k] = have ? s_row[k * KT_THREADS + tid] : 0.0;
            }
            if (valid != nullptr) valid[(size_t)b * M + j] = (unsigned char)ok;
        }
        // exclusive prefix of the lengths in candidate order
        int inc = len;
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) s_wsum[wave] = inc;
        s_len[tid] = len;
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int w = 0; w < KT_WAVES; ++w) {
            if (w < wave) woff += s_wsum[w];
            total += s_wsum[w];
        }
        s_off[tid] = base + woff + inc - len;
        __syncthreads();
        for (int l = wave; l < KT_THREADS; l += KT_WAVES) {
            const int ll = s_len[l];
            const unsigned char* src = s_line + l * KT_SLOT;
            unsigned char* dst = out + s_off[l];
            for (int k = lane; k < ll; k += 64) dst[k] = src[k];
        }
        base += total;
        __syncthreads();
    }
    if (flag) atomicOr(&s_flag, flag);
    __syncthreads();
    if (tid == 0) {
        const int f = s_flag;
        status[b] = (f & 2) ? 2 : (f & 1);
        text_len[b] = f ? 0 : base;
    }
}

PRCNN_API int prcnn_kitti_result_text(const float* boxes, const float* scores, const int32_t* keep, const int32_t* num, int B, int M,
                                      const double* P2, const int32_t* img_hw, const char* class_name, uint8_t* text, int32_t* text_len,
                                      int32_t* status, double* rows, uint8_t* valid, prcnn_stream_t stream) {
    PRCNN_REQUIRE(B >= 0 && M >= 0, "prcnn_kitti_result_text: bad sizes B=%d M=%d", B, M);
    PRCNN_REQUIRE(B <= 65535 && M <= (1 << 20), "prcnn_kitti_result_text: B=%d (<= 65535) or M=%d (<= 2^20) too large", B, M);
    PRCNN_REQUIRE(class_name != nullptr, "prcnn_kitti_result_text: null class name");
    size_t cl = 0;
    while (cl <= KT_CLASS_MAX && class_name[cl] != '\0') ++cl;
    PRCNN_REQUIRE(cl >= 1 && cl <= KT_CLASS_MAX, "prcnn_kitti_result_text: the class name must have 1 to %d bytes", KT_CLASS_MAX);
    if (B == 0 || M == 0) return PRCNN_OK;
    PRCNN_REQUIRE(boxes && scores && P2 && img_hw && text && text_len && status, "prcnn_kitti_result_text: null pointer");
    PRCNN_REQUIRE((uintptr_t)P2 % 8 == 0 && (rows == nullptr || (uintptr_t)rows % 8 == 0),
                  "prcnn_kitti_result_text: P2 and rows must be 8-byte aligned");
    KtClass cls = {{0u, 0u, 0u, 0u}, (int)cl};
    for (size_t k = 0; k < cl; ++k) cls.w[k >> 2] |= (uint32_t)(unsigned char)class_name[k] << (8 * (k & 3));
    hipLaunchKernelGGL(kitti_text_kernel, dim3((unsigned)B), dim3(KT_THREADS), 0, (hipStream_t)stream, boxes, scores, keep, num, M, P2,
                       img_hw, cls, text, text_len, status, rows, valid);
    PRCNN_LAUNCH_CHECK("prcnn_kitti_result_text");
    return PRCNN_OK;
}
