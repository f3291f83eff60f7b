// Stands in for <hip/hip_runtime.h> when a __host__ __device__ header of csrc/ is compiled by a plain host compiler for a CPU test.
#pragma once
#include <cmath>
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
