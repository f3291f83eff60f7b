// level_units.h -- a launch that carries several problems: which problem a workgroup works on, and how a bounded number of
// workgroups is dealt to the problems.  Plain code (no HIP call): the kernels of mlp_multi.h and the host launcher use it, and
// tests/level_units_host.cpp compiles it for the host.
//
// The problems take consecutive runs of the 1-D grid, in the order given (heaviest first, so that the long problems start
// first and the short ones fill the tail).  A workgroup learns (problem, its index among that problem's workgroups, their
// number) and runs the problem's kernel body with the last two in the place of blockIdx.x / gridDim.x: a body that strides
// over its work units by its workgroup count visits every unit exactly once whatever share of the grid it was given, as long
// as a problem that has units has at least one workgroup.
#pragma once
#include <hip/hip_runtime.h>

#define LEVEL_MAX_PROBLEMS 4

struct LevelUnits {
    int nprob;
    int end[LEVEL_MAX_PROBLEMS];        // one past the last workgroup of problem p; end[nprob - 1] is the grid
};

__host__ __device__ __forceinline__ void level_units_find(const LevelUnits& U, int block, int& prob, int& local, int& count) {
    int first = 0;
    prob = 0;
    for (int p = 0; p + 1 < U.nprob; p++)
        if (block >= U.end[p]) { prob = p + 1; first = U.end[p]; }
    local = block - first;
    count = U.end[prob] - first;
}

// want[p]: the grid problem p would be launched with on its own (0: nothing to do).  cap <= 0 or sum(want) <= cap: every
// problem keeps its own grid.  Otherwise the cap is divided in proportion to weight[p] (null: want[p]) among the problems that
// want any: never more than want[p], never less than 1, what rounding leaves over goes to the problems in order.  Returns the
// grid (0: no problem has work), or -1 when the cap is smaller than the number of problems that have work.
static inline long level_units_share(LevelUnits& U, const long* want, const long* weight, int nprob, long cap) {
    long g[LEVEL_MAX_PROBLEMS] = {0, 0, 0, 0};
    if (nprob < 1 || nprob > LEVEL_MAX_PROBLEMS) return -1;
    long sum = 0, wsum = 0;
    int live = 0;
    for (int p = 0; p < nprob; p++) {
        if (want[p] < 0 || want[p] > (1L << 31) || (weight && (weight[p] < 0 || weight[p] > (1L << 40))) || cap > (1L << 21)) return -1;
        if (want[p] == 0) continue;
        live++;
        sum += want[p];
        wsum += weight ? (weight[p] > 0 ? weight[p] : 1) : want[p];
    }
    if (cap <= 0 || sum <= cap) {
        for (int p = 0; p < nprob; p++) g[p] = want[p];
    } else {
        if (cap < live) return -1;
        // one workgroup each first, the rest of the cap in proportion (rounded down, clipped to what the problem wants)
        long left = cap - live;
        for (int p = 0; p < nprob; p++) {
            if (want[p] == 0) continue;
            const long w = weight ? (weight[p] > 0 ? weight[p] : 1) : want[p];
            long extra = (cap - live) * w / wsum;             // (< 2^62: checked above)
            if (extra > want[p] - 1) extra = want[p] - 1;
            g[p] = 1 + extra;
            left -= extra;
        }
        for (int p = 0; p < nprob && left > 0; p++) {
            const long more = want[p] - g[p] < left ? want[p] - g[p] : left;
            if (want[p] == 0 || more <= 0) continue;
            g[p] += more;
            left -= more;
        }
    }
    long at = 0;
    U.nprob = nprob;
    for (int p = 0; p < LEVEL_MAX_PROBLEMS; p++) {
        if (p < nprob) at += g[p];
        if (at > 2147483647L) return -1;
        U.end[p] = (int)at;
    }
    return at;
}
