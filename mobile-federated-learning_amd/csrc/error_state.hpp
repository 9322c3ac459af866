// error_state.hpp -- the last-error message of one native library (HIP-free;
// also g++-built by tests/native/error_state_check.cpp).
//
// Each library keeps one `thread_local ErrorState` and returns its c_str()
// from its *_last_error(): a message belongs to the thread whose call failed
// and stays until that thread's next failure or successful launch.
// launch_status (common.hpp) is the HIP side.
#pragma once

#include <cstdarg>
#include <cstdio>

namespace fedavg_impl {

// Hidden: the inline members never join a library's dynamic symbols.
struct __attribute__((visibility("hidden"))) ErrorState {
  char text[512] = "";

  // printf-style; a longer message is cut at the buffer's end.  Returns `code`.
  int vset(int code, const char* fmt, va_list ap) {
    std::vsnprintf(text, sizeof(text), fmt, ap);
    return code;
  }
  int set(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
    va_list ap;
    va_start(ap, fmt);
    vset(code, fmt, ap);
    va_end(ap);
    return code;
  }
  void clear() { text[0] = '\0'; }
  const char* c_str() const { return text; }
};

}  // namespace fedavg_impl
