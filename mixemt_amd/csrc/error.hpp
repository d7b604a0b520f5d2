// error.hpp -- part of libmixemt_hip.so; host only (no HIP header, no device compiler needed for fail itself).
// The calling thread's last error message (mxm_last_error) and the one way to set it.
#ifndef MIXEMT_ERROR_HPP
#define MIXEMT_ERROR_HPP

#include <stdarg.h>
#include <stdio.h>

static thread_local char g_err[512] = "";

// Writes the message and returns `code`.  The format is checked against its arguments at compile time (the build
// makes -Wformat an error): an int32_t goes to %d, or is cast to long long for %lld.
__attribute__((format(printf, 2, 3))) static int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// (for translation units that include hip_runtime.h)
#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) return fail(-2, "HIP error: %s (line %d)", hipGetErrorString(e_), __LINE__); \
    } while (0)

#endif  // MIXEMT_ERROR_HPP
