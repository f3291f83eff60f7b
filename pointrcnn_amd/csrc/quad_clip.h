// quad_clip.h -- the overlap of two box corner sets as kitti_utils.get_iou3d computes it (lib/utils/kitti_utils.py:195-235),
// with shapely's polygon intersection restated as an exact convex clip in DOUBLE precision.
//
// This is deliberately separate from iou3d_geom.h / ref_trig.h: those restate the reference's CUDA fp32 arithmetic; shapely works
// in double, so every step below after the height test is double.
//
//   heights (fp32, as numpy does them): min_h = -(((y0 + y1) + y2) + y3) / 4 over corners 0:4, max_h likewise over 4:8;
//                                       h = max(0, min(max_h) - max(min_h)); h == 0 -> IoU 0 (the reference skips the pair)
//   bottom polygons: corners 0:4 in (x, z), cast to double.  A quad is valid iff it is strictly convex (its four turns have one
//                    strict sign): shapely's is_valid branch gives 0 for degenerate / self-intersecting quads, and so does this
//                    (a simple but concave quad, which no box produces, is also treated as invalid here).
//   overlap: Sutherland-Hodgman clip of a by b's four half-planes (both oriented counter-clockwise), shoelace area, all double;
//   iou3d = o*h / (area_a*dh_a + area_b*dh_b - o*h), iou_bev = o / (area_a + area_b - o), stored as fp32.
#pragma once
#include <hip/hip_runtime.h>

constexpr int QC_MAX_VERTS = 16;          // a convex clip of a quad by four half-planes has <= 8; the guard absorbs rounding

struct QcQuad {
    double x[4], z[4];
    double area;                          // > 0 for a valid quad, 0 otherwise
};

__host__ __device__ __forceinline__ double qc_cross(double ax, double az, double bx, double bz, double px, double pz) {
    return (bx - ax) * (pz - az) - (bz - az) * (px - ax);
}

// shoelace over n vertices in order, |.| / 2
__host__ __device__ inline double qc_shoelace(const double* x, const double* z, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 == n ? 0 : i + 1;
        s = s + (x[i] * z[j] - x[j] * z[i]);
    }
    return fabs(s) * 0.5;
}

// (x, z) of corners 0:4 (fp32, stride 3 floats per corner: the (8,3) corner layout) -> a counter-clockwise quad, area 0 if invalid
__host__ __device__ inline QcQuad qc_make(const float* c) {
    QcQuad q;
    double x[4], z[4];
    for (int k = 0; k < 4; ++k) {
        x[k] = (double)c[3 * k + 0];
        z[k] = (double)c[3 * k + 2];
    }
    int pos = 0, neg = 0;
    for (int k = 0; k < 4; ++k) {
        const int a = k, b = (k + 1) & 3, n = (k + 2) & 3;
        const double t = qc_cross(x[a], z[a], x[b], z[b], x[n], z[n]);
        pos += t > 0.0;
        neg += t < 0.0;
    }
    const bool flip = neg == 4;
    for (int k = 0; k < 4; ++k) {
        const int s = flip ? 3 - k : k;
        q.x[k] = x[s];
        q.z[k] = z[s];
    }
    q.area = (pos == 4 || neg == 4) ? qc_shoelace(q.x, q.z, 4) : 0.0;
    return q;
}

// area of a ∩ b for two valid counter-clockwise quads
__host__ __device__ inline double qc_overlap(const QcQuad& a, const QcQuad& b) {
    double px[QC_MAX_VERTS], pz[QC_MAX_VERTS], qx[QC_MAX_VERTS], qz[QC_MAX_VERTS];
    int n = 4;
    for (int k = 0; k < 4; ++k) {
        px[k] = a.x[k];
        pz[k] = a.z[k];
    }
    for (int e = 0; e < 4 && n > 0; ++e) {
        const double ex0 = b.x[e], ez0 = b.z[e], ex1 = b.x[(e + 1) & 3], ez1 = b.z[(e + 1) & 3];
        int m = 0;
        double sp = qc_cross(ex0, ez0, ex1, ez1, px[n - 1], pz[n - 1]);
        for (int i = 0; i < n; ++i) {
            const int j = i == 0 ? n - 1 : i - 1;
            const double sc = qc_cross(ex0, ez0, ex1, ez1, px[i], pz[i]);
            if ((sc >= 0.0) != (sp >= 0.0) && m < QC_MAX_VERTS) {
                const double t = sp / (sp - sc);
                qx[m] = px[j] + t * (px[i] - px[j]);
                qz[m] = pz[j] + t * (pz[i] - pz[j]);
                ++m;
            }
            if (sc >= 0.0 && m < QC_MAX_VERTS) {
                qx[m] = px[i];
                qz[m] = pz[i];
                ++m;
            }
            sp = sc;
        }
        n = m;
        for (int i = 0; i < n; ++i) {
            px[i] = qx[i];
            pz[i] = qz[i];
        }
    }
    return n < 3 ? 0.0 : qc_shoelace(px, pz, n);
}

// fp32 height range of one corner set (8,3): lo = min_h, hi = max_h
__host__ __device__ __forceinline__ void qc_heights(const float* c, float& lo, float& hi) {
    lo = -(((c[1] + c[4]) + c[7]) + c[10]) / 4.0f;
    hi = -(((c[13] + c[16]) + c[19]) + c[22]) / 4.0f;
}

// fp32 height overlap of two ranges (0 -> the reference skips the pair)
__host__ __device__ __forceinline__ float qc_h_overlap(float lo_a, float hi_a, float lo_b, float hi_b) {
    const float v = fminf(hi_a, hi_b) - fmaxf(lo_a, lo_b);
    return v > 0.0f ? v : 0.0f;
}

// the pair's iou3d / iou_bev given the height ranges, quads and h > 0
__host__ __device__ inline void qc_ratios(const QcQuad& a, const QcQuad& b, float h, float dh_a, float dh_b, float& iou3d, float& bev) {
    if (a.area == 0.0 || b.area == 0.0) {
        iou3d = 0.0f;
        bev = 0.0f;
        return;
    }
    const double o = qc_overlap(a, b);
    const double o3 = o * (double)h;
    iou3d = (float)(o3 / ((a.area * (double)dh_a + b.area * (double)dh_b) - o3));
    bev = (float)(o / ((a.area + b.area) - o));
}
