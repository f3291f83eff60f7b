// head_tail_math.h -- the Dropout mask of the training heads' tail (head_tail.hip), host and device: a pure function of a key and the
// entry's position, so that backward rebuilds what forward drew and a resumed run replays the masks of the run it continues.
//   keep(seed, stream, call, r, k) = scene_u01f(scene_rand(seed, stream, call, r * K + k)) >= p        (counter_rand.h; call sits in
//   scale = 1.0f / (1.0f - p)                                                                           the generator's frame slot)
// p is float32, 0 <= p < 1; the comparison is a float32 one.  r * K + k is taken modulo 2^32 (the domain is R * K <= 2^32, every entry
// its own counter).  p == 0 keeps every entry (u01 >= 0) with scale exactly 1.  Stream ids: 70 + the Dropout module's ordinal
// (scene.hip's header comment lists the ids in use).
// A dropped entry is SELECTED to zero, never multiplied by zero: an Inf or NaN in a dropped position of x contributes nothing, where
// torch's x * mask gives NaN.  The Python twin is pointrcnn_amd.train_mlp.head_keep_mask.
#pragma once
#include "counter_rand.h"

// the part of scene_rand that does not depend on the entry: scene_rand(seed, stream, call, i) == scene_mix(i ^ head_tail_key(...))
__host__ __device__ __forceinline__ unsigned head_tail_key(unsigned seed, unsigned stream, unsigned call) {
    return scene_mix(call * 0x9E3779B9U + scene_mix(seed + stream * 0x85EBCA6BU));
}
__host__ __device__ __forceinline__ bool head_tail_keep_i(unsigned key, unsigned i, float p) { return scene_u01f(scene_mix(i ^ key)) >= p; }
__host__ __device__ __forceinline__ bool head_tail_keep(unsigned seed, unsigned stream, unsigned call, unsigned long long r, unsigned K,
                                                        unsigned k, float p) {
    return scene_u01f(scene_rand(seed, stream, call, (unsigned)(r * K + k))) >= p;
}
__host__ __device__ __forceinline__ float head_tail_scale(float p) { return 1.0f / (1.0f - p); }
// drop(x): the kept entry scaled, the dropped one selected to zero
__host__ __device__ __forceinline__ float head_tail_drop(float x, bool keep, float scale) { return keep ? x * scale : 0.0f; }
