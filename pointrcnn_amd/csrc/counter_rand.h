// counter_rand.h -- the counter-based generator of the input builders (scene.hip, train_input.hip), one definition for both:
//   r(stream, frame, i) = mix(i ^ mix(frame * 0x9E3779B9 + mix(seed + stream * 0x85EBCA6B))),  mix = the 32-bit finaliser below.
// The stream ids in use are listed in scene.hip's header comment.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ unsigned scene_mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__host__ __device__ __forceinline__ unsigned scene_rand(unsigned seed, unsigned stream, unsigned frame, unsigned i) {
    return scene_mix(i ^ scene_mix(frame * 0x9E3779B9U + scene_mix(seed + stream * 0x85EBCA6BU)));
}
// u01(r) = fp32(r >> 8) * 2^-24: the uniform draw behind every np.random.rand() / uniform() of the table, as the float32 it is (the
// online RoI sampler's noise is float32 arithmetic) and widened to double
__host__ __device__ __forceinline__ float scene_u01f(unsigned r) { return (float)(r >> 8) * (1.0f / 16777216.0f); }
__host__ __device__ __forceinline__ double scene_u01(unsigned r) { return (double)scene_u01f(r); }
