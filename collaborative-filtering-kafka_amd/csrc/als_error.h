// als_error.h -- the library's one error report (als_error.cpp), for every unit, host-only or not. Private to csrc/.
#pragma once

namespace cfk_detail {
// Sets the thread's als_last_error() message and returns `code`.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
}  // namespace cfk_detail
