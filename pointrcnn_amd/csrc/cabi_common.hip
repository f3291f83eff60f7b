// cabi_common.hip -- error reporting, version and the environment-switch snapshot for the C ABI (include/prcnn_pointops.h).
#include "common.h"
#define PRCNN_SWITCHES_IMPLEMENTATION
#include "switches.h"
#include <stdarg.h>

static thread_local char g_err[512] = "";

int prcnn_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

PRCNN_API const char* prcnn_last_error(void) { return g_err; }
PRCNN_API int prcnn_abi_version(void) { return 12; }

#ifndef PRCNN_BUILD_ID
#define PRCNN_BUILD_ID "PRCNN_BUILD_ID=unknown"
#endif
// the macro carries the "PRCNN_BUILD_ID=" tag so that the digest can also be read from the file without loading it
PRCNN_API const char* prcnn_build_id(void) { return &PRCNN_BUILD_ID[sizeof("PRCNN_BUILD_ID=") - 1]; }

PRCNN_API int prcnn_switches_reload(void) {
    prcnn_switch_reload();
    return PRCNN_OK;
}
PRCNN_API int prcnn_switch_get(const char* name, int* set, long* num) {
    const int i = prcnn_switch_find(name);
    PRCNN_REQUIRE(i >= 0, "prcnn_switch_get: %s is not a switch of this library (csrc/switches.h)", name ? name : "(null)");
    const PrcnnSwitchValue& v = sw_value((PrcnnSwitch)i);
    if (set) *set = v.set;
    if (num) *num = v.num;
    return PRCNN_OK;
}
