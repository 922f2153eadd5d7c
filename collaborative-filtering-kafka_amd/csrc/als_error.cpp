// als_error.cpp -- the thread's last error message (als_error.h) and als_last_error of include/als.h. No HIP header.
#include "als_error.h"

#include <cstdarg>
#include <cstdio>
#include <string>

#include "als.h"

static thread_local std::string g_last_error;

int cfk_detail::fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

extern "C" const char* als_last_error(void) { return g_last_error.c_str(); }
