// Recording prelude of the stand-alone launch recorders (tests/mlp_launch_record.cpp, tests/train_launch_record.cpp): csrc/mlp.hip is
// compiled as HIP host code only, the device queries answer "device 0, 256 CUs", and the launch macro records the kernel instance,
// grid, block and dynamic LDS instead of launching.  Included before MLP_SOURCE; the including program defines rec_params().
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <string>
#include <typeinfo>
#include <vector>
#define hipGetDevice(p) (*(p) = 0, hipSuccess)
#define hipDeviceGetAttribute(p, a, d) (*(p) = 256, hipSuccess)
#define hipFuncSetAttribute(f, a, v) ((void)(f), hipSuccess)
#define hipGetLastError() hipSuccess
#define PRCNN_SWITCHES_IMPLEMENTATION
#include "switches.h"
#include "common.h"

// host-only HIP code still registers its (absent) device code at start-up: these stand in for the runtime's entry points, so that
// none of it runs (the program is linked with --unresolved-symbols=ignore-all for the fat binary that does not exist)
extern "C" void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
extern "C" void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
extern "C" void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
extern "C" void __hipUnregisterFatBinary(void**) {}

static std::string g_rec;            // the record of the call in flight
static int g_launches = 0;
static void recf(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_rec += buf;
}
int prcnn_fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_rec += " !";
    g_rec += buf;
    return code;
}

// names a kernel by its instantiation: the mangled name of KName<&kernel<args>> spells the template arguments out
template <auto K> struct KName {
    static const std::string& get() {
        static const std::string name = [] {
            std::string s = typeid(KName<K>).name();
            for (size_t i; (i = s.find("__device_stub__")) != std::string::npos;) s.erase(i, strlen("__device_stub__"));
            return s;
        }();
        return name;
    }
};
struct MlpParams;
struct ChainParams;
static void rec_params(const MlpParams& P);
static void rec_params(const ChainParams& C);
static void rec_head(const std::string& k, dim3 g, dim3 b, size_t lds) {
    g_launches++;
    recf(" | %s grid %u,%u,%u block %u,%u,%u lds %zu", k.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
}
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const MlpParams& P) { rec_head(k, g, b, lds); rec_params(P); }
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const MlpParams& P, int split_max) {
    rec_head(k, g, b, lds);
    rec_params(P);
    recf(" split_max %d", split_max);
}
static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const ChainParams& C) { rec_head(k, g, b, lds); rec_params(C); }
template <class... A> static void rec_launch(const std::string& k, dim3 g, dim3 b, size_t lds, const A&...) { rec_head(k, g, b, lds); }
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) rec_launch(KName<kernel>::get(), grid, block, lds, __VA_ARGS__)
