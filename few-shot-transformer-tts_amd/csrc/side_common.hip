// side_common.h: host code only, compiled once into every satellite library.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <string>
#include "side_common.h"

namespace {
thread_local std::string g_err;
}

namespace b2s_side {

int fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

const char *last_error() { return g_err.c_str(); }

int launch_status(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: launch failed: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace b2s_side
