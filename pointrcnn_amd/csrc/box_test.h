// box_test.h -- the analytic point-in-box test of roipool3d (roipool3d.cpp:82-95), one definition for every kernel that asks
// whether a point lies in a box: roipool3d.hip (pooling, pts_in_boxes3d, RPN labels, GT-augmentation edit) and train_scene.hip.
#pragma once
#include "common.h"
#include "ref_trig.h"

struct BoxConst { float cx, cy, cz, hh, hw, hl, cosa, sina; };

__device__ __forceinline__ BoxConst make_box(const float* bx) {
    // roipool3d.cpp:82-95.  cy = bottom_y - h/2 in double then rounded (exactly what the reference's
    // `h / 2.0` expression does); cos/sin as the reference's host libm evaluates cos(float) / sin(float) (ref_trig.h:
    // glibc's routines restated bit for bit -- points on a box face land on the reference's side of it).
    BoxConst b;
    b.cx = bx[0]; b.cz = bx[2];
    b.cy = (float)((double)bx[1] - (double)bx[3] / 2.0);
    b.hh = bx[3] * 0.5f; b.hw = bx[4] * 0.5f; b.hl = bx[5] * 0.5f;      // exact halvings
    b.cosa = prcnn_ref_cosf(bx[6]);
    b.sina = prcnn_ref_sinf(bx[6]);
    return b;
}

// GATE: the reference's pt_in_box3d rejects any point further than max_dis = 10 m from the centre in x or z before it rotates
// (roipool3d.cpp:87-89, roipool3d_kernel.cu:19-21) -- part of roipool3d / pts_in_boxes3d semantics.  The label generator is a
// hull test on the box corners with no such limit (kitti_rcnn_dataset.py:365-394): GATE = false.
template <bool GATE = true>
__device__ __forceinline__ bool pt_in_box(const BoxConst& b, float x, float y, float z) {
    if (fabsf(y - b.cy) > b.hh) return false;
    if (GATE && (fabsf(x - b.cx) > 10.0f || fabsf(z - b.cz) > 10.0f)) return false;
    float dx = x - b.cx, dz = z - b.cz;
    float x_rot = __fadd_rn(__fmul_rn(dx, b.cosa), __fmul_rn(dz, -b.sina));
    float z_rot = __fadd_rn(__fmul_rn(dx, b.sina), __fmul_rn(dz, b.cosa));
    return (x_rot >= -b.hl) & (x_rot <= b.hl) & (z_rot >= -b.hw) & (z_rot <= b.hw);
}
