// Stand-alone host program (no HIP): every native switch, through the accessor its call site uses, against the getenv
// expression that call site held before the switches moved into csrc/switches.h.  The legacy expressions are written out
// literally, as they stood in fps.hip / mlp.hip / gather.hip / proposal.hip / mlp_train.h.  Built and run by
// tests/test_switches_cpu.py (once plain, once with -fsanitize=address,undefined).
#define PRCNN_SWITCHES_IMPLEMENTATION
#include "switches.h"
#include <stdio.h>

struct Case {
    PrcnnSwitch id;
    const char* site;
    long (*now)();
    long (*legacy)();
};

static const Case CASES[] = {
    {SW_FPS_SLOTS, "fps.hip: slots", [] { return (long)sw_enabled(SW_FPS_SLOTS); },
     [] { const char* slots_env = getenv("PRCNN_FPS_SLOTS"); return (long)(slots_env == nullptr || atoi(slots_env) != 0); }},
    {SW_FPS_BATCH, "fps.hip: batch", [] { return (long)sw_opt_in(SW_FPS_BATCH); },
     [] { const char* batch_env = getenv("PRCNN_FPS_BATCH"); return (long)(batch_env != nullptr && atoi(batch_env) != 0); }},
    {SW_FPS_MEM, "fps.hip: use_mem", [] { return (long)sw_present(SW_FPS_MEM); }, [] { return (long)(getenv("PRCNN_FPS_MEM") != nullptr); }},
    {SW_CHAIN_PERSIST, "mlp.hip: chain_persist_on", [] { return (long)sw_enabled(SW_CHAIN_PERSIST); },
     [] { const char* e = getenv("PRCNN_CHAIN_PERSIST"); return (long)!(e && atoi(e) == 0); }},
    {SW_CHAIN_COOP, "mlp.hip: chain_coop_on", [] { return (long)(sw_num(SW_CHAIN_COOP, 1) != 0); },
     [] { const char* e = getenv("PRCNN_CHAIN_COOP"); return (long)!(e && atoi(e) == 0); }},
    {SW_CHAIN_COOP, "mlp.hip: chain_coop_forced", [] { return (long)(sw_num(SW_CHAIN_COOP, 1) == 2); },
     [] { const char* e = getenv("PRCNN_CHAIN_COOP"); return (long)(e && atoi(e) == 2); }},
    {SW_SPLIT_MIN_TILES, "mlp.hip: split_min", [] { return sw_num(SW_SPLIT_MIN_TILES, 0); },
     [] { return (long)(getenv("PRCNN_SPLIT_MIN_TILES") ? atol(getenv("PRCNN_SPLIT_MIN_TILES")) : 0); }},
    {SW_GROUP_SPLIT, "mlp.hip: group_split_on", [] { return (long)sw_enabled(SW_GROUP_SPLIT); },
     [] { return (long)!(getenv("PRCNN_GROUP_SPLIT") && atoi(getenv("PRCNN_GROUP_SPLIT")) == 0); }},
    {SW_SPLIT_WIDE_MIN, "mlp.hip: split_wide_min", [] { return sw_num(SW_SPLIT_WIDE_MIN, 192); },
     [] { return (long)(getenv("PRCNN_SPLIT_WIDE_MIN") ? atol(getenv("PRCNN_SPLIT_WIDE_MIN")) : 192); }},
    {SW_BOUNDED_GRID, "mlp.hip: bounded_on", [] { return (long)sw_enabled(SW_BOUNDED_GRID); },
     [] { return (long)!(getenv("PRCNN_BOUNDED_GRID") && atoi(getenv("PRCNN_BOUNDED_GRID")) == 0); }},
    {SW_WIDE_MIN_TILES, "mlp.hip: wide_min", [] { return sw_num(SW_WIDE_MIN_TILES, 192); },
     [] { return (long)(getenv("PRCNN_WIDE_MIN_TILES") ? atol(getenv("PRCNN_WIDE_MIN_TILES")) : 192); }},
    {SW_WIDE_MIN_TILES, "mlp.hip: v2 tile rule", [] { return (long)!sw_present(SW_WIDE_MIN_TILES); },
     [] { return (long)(getenv("PRCNN_WIDE_MIN_TILES") == nullptr); }},
    {SW_WIDE_LISTS, "mlp.hip: wide_lists", [] { return (long)sw_present(SW_WIDE_LISTS); }, [] { return (long)(getenv("PRCNN_WIDE_LISTS") != nullptr); }},
    {SW_LAYER_V1, "mlp.hip: force_v1", [] { return (long)sw_present(SW_LAYER_V1); }, [] { return (long)(getenv("PRCNN_LAYER_V1") != nullptr); }},
    {SW_NO_WGM, "mlp.hip: wgm", [] { return (long)!sw_present(SW_NO_WGM); }, [] { return (long)(getenv("PRCNN_NO_WGM") == nullptr); }},
    {SW_ADDY_PHASE, "mlp.hip: addy_phase", [] { return (long)(int)sw_num(SW_ADDY_PHASE, 2); },
     [] { return (long)(getenv("PRCNN_ADDY_PHASE") ? atoi(getenv("PRCNN_ADDY_PHASE")) : 2); }},
    {SW_NO_ROWS32, "mlp.hip: rows32 off", [] { return (long)sw_present(SW_NO_ROWS32); }, [] { return (long)(getenv("PRCNN_NO_ROWS32") != nullptr); }},
    {SW_NO_STACK, "mlp.hip: stack offered", [] { return (long)!sw_present(SW_NO_STACK); }, [] { return (long)(getenv("PRCNN_NO_STACK") == nullptr); }},
    {SW_NO_SA0, "mlp.hip: sa0", [] { return (long)!sw_present(SW_NO_SA0); }, [] { return (long)(getenv("PRCNN_NO_SA0") == nullptr); }},
    {SW_PERSISTENT_CHAIN, "mlp.hip: persistent chain", [] { return (long)sw_present(SW_PERSISTENT_CHAIN); },
     [] { return (long)(getenv("PRCNN_PERSISTENT_CHAIN") != nullptr); }},
    {SW_NO_FAST_CHAIN, "mlp.hip: fast chain", [] { return (long)!sw_present(SW_NO_FAST_CHAIN); },
     [] { return (long)(getenv("PRCNN_NO_FAST_CHAIN") == nullptr); }},
    {SW_NO_XCD_ORDER, "mlp.hip: xcd order", [] { return (long)!sw_present(SW_NO_XCD_ORDER); },
     [] { return (long)(getenv("PRCNN_NO_XCD_ORDER") == nullptr); }},
    {SW_GATHER_DIRECT, "gather.hip: direct", [] { return (long)sw_present(SW_GATHER_DIRECT); },
     [] { return (long)(getenv("PRCNN_GATHER_DIRECT") != nullptr); }},
    {SW_INTERP_DIRECT, "gather.hip: no_lds", [] { return (long)sw_present(SW_INTERP_DIRECT); },
     [] { return (long)(getenv("PRCNN_INTERP_DIRECT") != nullptr); }},
    {SW_INTERP_LAYOUT, "gather.hip: lds rows", [] { return (long)(sw_c0(SW_INTERP_LAYOUT) == 'r'); },
     [] { const char* lay = getenv("PRCNN_INTERP_LAYOUT"); return (long)(lay && lay[0] == 'r'); }},
    {SW_INTERP_CGT, "gather.hip: CGT 4", [] { return (long)(sw_num(SW_INTERP_CGT, 0) == 4); },
     [] { const char* cge = getenv("PRCNN_INTERP_CGT"); return (long)(cge && atoi(cge) == 4); }},
    {SW_TRAIN_FWD_GENERIC, "mlp_train.h: fastp", [] { return (long)!sw_present(SW_TRAIN_FWD_GENERIC); },
     [] { return (long)!getenv("PRCNN_TRAIN_FWD_GENERIC"); }},
    {SW_WGRAD_DIRECT, "mlp_train.h: wgrad lds", [] { return (long)!sw_present(SW_WGRAD_DIRECT); }, [] { return (long)!getenv("PRCNN_WGRAD_DIRECT"); }},
    {SW_NMS_PREFILTER, "proposal.hip: prefilter", [] { return (long)sw_enabled(SW_NMS_PREFILTER); },
     [] { const char* e = getenv("PRCNN_NMS_PREFILTER"); return (long)(e == nullptr || atoi(e) != 0); }},
};

static int failures = 0;
static void expect(bool ok, const char* what, const char* name, const char* value) {
    if (ok) return;
    failures++;
    printf("FAIL %s: %s=%s\n", what, name, value ? value : "(unset)");
}

static void put(const char* name, const char* value) {
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}

int main() {
    static const char* const VALUES[] = {nullptr, "", "0", "1", "2", "4", "-1", "rows", "abc"};
    bool covered[SW_COUNT] = {};
    for (const Case& c : CASES) covered[c.id] = true;
    for (int i = 0; i < SW_COUNT; i++) {
        expect(covered[i], "no case for this table entry", prcnn_switch_names[i], nullptr);
        expect(prcnn_switch_find(prcnn_switch_names[i]) == i, "prcnn_switch_find", prcnn_switch_names[i], nullptr);
        put(prcnn_switch_names[i], nullptr);
    }
    expect(!sw_value(SW_FPS_SLOTS).set && sw_enabled(SW_FPS_SLOTS), "first use takes the snapshot", prcnn_switch_names[SW_FPS_SLOTS], nullptr);
    expect(prcnn_switch_find("PRCNN_NO_SUCH_SWITCH") == -1 && prcnn_switch_find(nullptr) == -1, "prcnn_switch_find of an unknown name", "-", nullptr);
    for (int i = 0; i < SW_COUNT; i++) {
        const char* name = prcnn_switch_names[i];
        for (const char* value : VALUES) {
            put(name, value);
            prcnn_switch_reload();
            const PrcnnSwitchValue& v = sw_value((PrcnnSwitch)i);
            expect(v.set == (value != nullptr) && v.num == (value ? atol(value) : 0) && v.c0 == (value ? value[0] : 0), "snapshot", name, value);
            for (const Case& c : CASES)          // the switch under test and, all unset, every other one
                expect(c.now() == c.legacy(), c.site, name, value);
        }
        // the snapshot is what launches read: a changed environment is seen after a reload, and only then
        put(name, "1");
        prcnn_switch_reload();
        put(name, "0");
        expect(sw_value((PrcnnSwitch)i).set && sw_value((PrcnnSwitch)i).num == 1, "value frozen until the reload", name, "1 -> 0");
        prcnn_switch_reload();
        expect(sw_value((PrcnnSwitch)i).set && sw_value((PrcnnSwitch)i).num == 0, "reload picks up the new value", name, "0");
        put(name, nullptr);
        prcnn_switch_reload();
        expect(!sw_value((PrcnnSwitch)i).set, "reload picks up the removal", name, nullptr);
    }
    printf("%d switches, %d call sites, %d failures\n", (int)SW_COUNT, (int)(sizeof(CASES) / sizeof(CASES[0])), failures);
    return failures ? 1 : 0;
}
