// aug_scene_math.h -- the per-try arithmetic of the offline GT-augmented scene generator (aug_scene.hip), host and device:
// AugSceneGenerator.aug_one_scene of tools/generate_aug_scene.py:149-233.  tests/aug_scene_host.cpp runs it on the host against the
// numpy twin (tests/aug_scene_twin.py).  The pair IoU between the range check and the accept decision is iou3d_pair.h (device only).
// What the loop fixes, and where it differs from the online loop of train_input.hip (apply_gt_aug_to_one_scene):
//   extra_gt_num = randint(10, 15) = 10 + below(r(60, frame, 0), 5): 10..14, no cfg feeds it                                  (:157)
//   try t (0-based, every started try counts, 50 of them): index = randint(0, D - 1) = below(r(61, frame, t), D - 1): the last
//   database entry is never drawn; D <= 1 raises                                                                               (:175)
//   the range check compares the float32 centre, widened, with the double bounds of PC_AREA_SCOPE                         (:138-147)
//   the plane move runs in double; the box's y is fp32(double(y) - move), a pasted point's y fp32(double(y) - move)      (:191-194)
//   list entries carry w + 0.5, l + 0.5 in float32; the NEW box is tested unenlarged                               (:161-162, :215-216)
//   accepted iff max IoU < 1e-8, float32 against float32 (numpy compares its float32 scalar with the Python float as float32)  (:201)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "counter_rand.h"

constexpr int AUGS_TRIES = 50;
constexpr int AUGS_MAX_ACCEPT = 15;        // cnt <= extra_gt_num + 1 <= 15 bounds the accepted objects
constexpr unsigned AUGS_STREAM_EXTRA = 60u, AUGS_STREAM_INDEX = 61u;

__host__ __device__ __forceinline__ int augs_below(unsigned r, int n) { return (int)(((unsigned long long)r * (unsigned long long)n) >> 32); }

__host__ __device__ __forceinline__ int augs_extra_num(unsigned seed, unsigned frame) {
    return 10 + augs_below(scene_rand(seed, AUGS_STREAM_EXTRA, frame, 0u), 5);
}

// D >= 2
__host__ __device__ __forceinline__ int augs_draw_index(unsigned seed, unsigned frame, int t, int D) {
    return augs_below(scene_rand(seed, AUGS_STREAM_INDEX, frame, (unsigned)t), D - 1);
}

__host__ __device__ __forceinline__ bool augs_in_scope(const float* c, const double* s) {
    const double x = c[0], y = c[1], z = c[2];
    return s[0] <= x && x <= s[1] && s[2] <= y && y <= s[3] && s[4] <= z && z <= s[5];
}

// put the box on the road plane a b c d: -> its new y; move = what a pasted point's y loses
__host__ __device__ __forceinline__ float augs_plane_move(const float* box, const double* pl, double& move) {
    const double cur_h = ((-pl[3] - pl[0] * (double)box[0]) - pl[2] * (double)box[2]) / pl[1];
    move = (double)box[1] - cur_h;
    return (float)((double)box[1] - move);
}

__host__ __device__ __forceinline__ float augs_point_y(float y, double move) { return (float)((double)y - move); }

__host__ __device__ __forceinline__ void augs_enlarge(const float* in, float* out) {
    for (int q = 0; q < 7; ++q) out[q] = in[q];
    out[4] = in[4] + 0.5f;
    out[5] = in[5] + 0.5f;
}

// one IoU of the new box against a list entry: a NaN collides (numpy's max propagates it and NaN < 1e-8 is false)
__host__ __device__ __forceinline__ bool augs_collides(float iou) { return !(iou < 1e-8f); }
