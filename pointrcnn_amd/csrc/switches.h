// switches.h -- every PRCNN_* environment variable the native library reads, in ONE table, read ONCE.
//
// Host only (no HIP header; compiles with a plain C++ compiler).  The environment is parsed into a snapshot on first
// use; launch paths only load from that snapshot.  prcnn_switches_reload() (include/prcnn_pointops.h) publishes a fresh
// snapshot: it is the one way to change a switch in a running process (pointrcnn_amd._cabi.switches).  Nothing else in
// csrc may call getenv.  The definitions live in cabi_common.hip, which defines PRCNN_SWITCHES_IMPLEMENTATION before
// including this file.
#pragma once
#include <atomic>
#include <stdlib.h>
#include <string.h>

// X(id, description): the variable is PRCNN_<id>.  All of these are A/B switches between kernels that give the same
// results; the rule each one is read by is the accessor at its call site (and the table in INTEGRATION.md).
#define PRCNN_SWITCHES(X)                                                                                              \
    X(FPS_SLOTS, "0: one-level pruned FPS kernel for 8192 < N <= 16384 instead of the two-level slot kernel")          \
    X(FPS_BATCH, "1: FPS kernel that takes two samples per exchange where the second is provable (8192 < N <= 16384)") \
    X(FPS_MEM, "set: N > 16384 FPS on the one-workgroup L2 re-read kernel instead of the multi-workgroup one")         \
    X(CHAIN_PERSIST, "0: split-bf16 chains on the per-tile kernels instead of the persistent one")                     \
    X(CHAIN_COOP, "0: split-bf16 chains on the lane-is-a-row kernel; 2: the cooperative form also for two-layer heads") \
    X(SPLIT_MIN_TILES, "n: launches of fewer than n split-bf16 tiles go to the fp32 layer kernels")                    \
    X(GROUP_SPLIT, "0: the hoisted grouped layer on the fp32 layer kernel instead of the split-bf16 one")              \
    X(SPLIT_WIDE_MIN, "n: least number of 128x128 tiles for which the split-bf16 layer takes the wide tile")           \
    X(BOUNDED_GRID, "0: one workgroup per tile of capacity for compacted lists instead of the bounded grid")           \
    X(WIDE_MIN_TILES, "n: least number of 128x128 tiles for which the fp32 layer takes the wide tile; set: no v2 tile rule") \
    X(WIDE_LISTS, "set: compacted row lists may take the wide fp32 tile")                                              \
    X(LAYER_V1, "set: the fp32 layer kernel that stages the B operand in LDS instead of v2")                           \
    X(NO_WGM, "set: no workgroup-to-tile remapping in the v2 fp32 layer kernel")                                       \
    X(ADDY_PHASE, "n: where the interpolated addend is fetched in the addend layer (0: all in the epilogue)")          \
    X(NO_ROWS32, "set: few-row wide layers on the layer kernel instead of the rows32 kernel")                          \
    X(NO_STACK, "set: prcnn_mlp_chain_supported does not offer the two-wide-layer stack kernel")                       \
    X(NO_SA0, "set: SA level 0 on the generic chain kernel instead of the register-weight kernel")                     \
    X(PERSISTENT_CHAIN, "set: fp32 chains on the weights-resident persistent kernel")                                  \
    X(NO_FAST_CHAIN, "set: fp32 chains on the generic chain kernel instead of the fast one")                           \
    X(NO_XCD_ORDER, "set: no XCD-aware tile order in the interpolating chains")                                        \
    X(GATHER_DIRECT, "set: gather on the plain kernel instead of the LDS-staged one")                                  \
    X(INTERP_DIRECT, "set: three_interp on the plain kernel instead of the LDS-staged ones")                           \
    X(INTERP_LAYOUT, "r...: three_interp stages channel-major LDS rows instead of point-major ones")                   \
    X(INTERP_CGT, "4: point-major three_interp takes 4 channels per workgroup")                                        \
    X(TRAIN_FWD_GENERIC, "set: training forward on the generic kernel instead of the plain fast form")                 \
    X(WGRAD_DIRECT, "set: weight gradient without the LDS-staged kernel")                                              \
    X(NMS_PREFILTER, "0: batched NMS on the greedy kernels without the overlap prefilter")

enum PrcnnSwitch {
#define X(id, desc) SW_##id,
    PRCNN_SWITCHES(X)
#undef X
    SW_COUNT
};

struct PrcnnSwitchValue {
    bool set;       // the variable is present
    char c0;        // its first character, 0 if unset
    long num;       // atol of its value, 0 if unset
};
struct PrcnnSwitchSnapshot {
    PrcnnSwitchValue v[SW_COUNT];
    const PrcnnSwitchSnapshot* older;       // the snapshot this one replaced: never freed, a concurrent launch may still be reading it
};

extern const char* const prcnn_switch_names[SW_COUNT];
extern std::atomic<const PrcnnSwitchSnapshot*> prcnn_switch_snapshot;
const PrcnnSwitchSnapshot* prcnn_switch_first_use();       // takes the first snapshot (any thread may get here first)
void prcnn_switch_reload();                                // publishes a fresh one (a few hundred bytes per reload stay allocated)
int prcnn_switch_find(const char* name);                   // index into the table, -1 for a name that is not in it

static inline const PrcnnSwitchValue& sw_value(PrcnnSwitch s) {
    const PrcnnSwitchSnapshot* p = prcnn_switch_snapshot.load(std::memory_order_acquire);
    if (!p) p = prcnn_switch_first_use();
    return p->v[s];
}
static inline bool sw_present(PrcnnSwitch s) { return sw_value(s).set; }
static inline bool sw_enabled(PrcnnSwitch s) { const PrcnnSwitchValue& v = sw_value(s); return !v.set || v.num != 0; }     // default on
static inline bool sw_opt_in(PrcnnSwitch s) { const PrcnnSwitchValue& v = sw_value(s); return v.set && v.num != 0; }       // default off
static inline long sw_num(PrcnnSwitch s, long dflt) { const PrcnnSwitchValue& v = sw_value(s); return v.set ? v.num : dflt; }
static inline char sw_c0(PrcnnSwitch s) { return sw_value(s).c0; }

#ifdef PRCNN_SWITCHES_IMPLEMENTATION
const char* const prcnn_switch_names[SW_COUNT] = {
#define X(id, desc) "PRCNN_" #id,
    PRCNN_SWITCHES(X)
#undef X
};
std::atomic<const PrcnnSwitchSnapshot*> prcnn_switch_snapshot{nullptr};

static PrcnnSwitchSnapshot* prcnn_switch_read_env() {
    PrcnnSwitchSnapshot* p = new PrcnnSwitchSnapshot();
    for (int i = 0; i < SW_COUNT; i++)
        if (const char* e = getenv(prcnn_switch_names[i])) p->v[i] = {true, e[0], atol(e)};
    return p;
}
const PrcnnSwitchSnapshot* prcnn_switch_first_use() {
    PrcnnSwitchSnapshot* fresh = prcnn_switch_read_env();
    const PrcnnSwitchSnapshot* seen = nullptr;
    if (prcnn_switch_snapshot.compare_exchange_strong(seen, fresh, std::memory_order_acq_rel)) return fresh;
    delete fresh;             // another thread published first; ours was never visible
    return seen;
}
void prcnn_switch_reload() {
    PrcnnSwitchSnapshot* fresh = prcnn_switch_read_env();
    fresh->older = prcnn_switch_snapshot.load(std::memory_order_acquire);
    while (!prcnn_switch_snapshot.compare_exchange_weak(fresh->older, fresh, std::memory_order_acq_rel)) {}
}
int prcnn_switch_find(const char* name) {
    for (int i = 0; name && i < SW_COUNT; i++)
        if (strcmp(name, prcnn_switch_names[i]) == 0) return i;
    return -1;
}
#endif
