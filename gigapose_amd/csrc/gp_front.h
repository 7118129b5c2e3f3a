// Host-side plumbing of a front-end ("side") library -- libgigapose_ingest / _rlestr / _onboard / _render / _texture / _eval / _dist / _refine / _verify / _maskfit / _shade / _gtinfo / _label / _coco / _appear.so -- written once:
// the thread-local message buffer behind <prefix>_last_error, the three return codes and the argument / launch checks of an
// entry point.  Header only: every library compiles its own copy into its own objects and links nothing of the others.
//   #define GP_FRONT_PREFIX gpi
//   #include "../gp_front.h"
// (The product library's gp_common.h keeps its own: it also carries GpProfScope and the status word.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#ifndef GP_FRONT_PREFIX
#error "define GP_FRONT_PREFIX (gpi, gps, gpo, gpr, gpt, gpe, gpd, gpf, gpv, gpm, gpl, gpg, gpa, gpc, gpp) before including gp_front.h"
#endif

#define GPF_OK 0
#define GPF_EINVAL -1
#define GPF_ELAUNCH -2

static thread_local char g_err[512] = "";
static void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

#define GPF_CAT2(a, b) a##b
#define GPF_CAT(a, b) GPF_CAT2(a, b)
extern "C" const char* GPF_CAT(GP_FRONT_PREFIX, _last_error)(void) { return g_err; }

#define GPF_REQUIRE(cond, ...)      \
    do {                            \
        if (!(cond)) {              \
            set_error(__VA_ARGS__); \
            return GPF_EINVAL;      \
        }                           \
    } while (0)

#define GPF_CHECK_HIP(name, call)                             \
    do {                                                      \
        hipError_t e_ = (call);                               \
        if (e_ != hipSuccess) {                               \
            set_error("%s: %s", name, hipGetErrorString(e_)); \
            return GPF_ELAUNCH;                               \
        }                                                     \
    } while (0)

#define GPF_CHECK_LAUNCH(name)                                               \
    do {                                                                     \
        hipError_t e_ = hipGetLastError();                                   \
        if (e_ != hipSuccess) {                                              \
            set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return GPF_ELAUNCH;                                              \
        }                                                                    \
    } while (0)

// N items on the grid's second dimension, H x W pixels indexed with an int
static inline bool frame_sizes_ok(int N, int H, int W) { return N >= 0 && N <= 65535 && H > 0 && W > 0 && (long long)H * W < (1ll << 31); }
