// The libraries' last-error state (csrc/error_state.hpp) under sanitizers
// (test infrastructure; no GPU).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       -I mobile-federated-learning_amd/csrc tests/native/error_state_check.cpp -o /tmp/error_state_check
//   /tmp/error_state_check                     (tests/test_native_sanitized.py runs it)
//
// What it checks, on a thread_local ErrorState as every library keeps one:
// (a) set() returns its code and stores the formatted text;
// (b) a message longer than the buffer is cut to 511 characters and
//     NUL-terminated, and nothing next to the buffer is written;
// (c) clear() empties the message;
// (d) two threads that fail at the same time each read back their own message.
// Exit status 0 = clean; any finding aborts (ASan/UBSan) or returns 1.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "error_state.hpp"

using fedavg_impl::ErrorState;

namespace {

int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

thread_local ErrorState g_err;

// the libraries' C-variadic setters forward like this
int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

std::atomic<int> arrived{0};
std::atomic<int> thread_failures{0};

void worker(int id) {
  const std::string mine = "thread " + std::to_string(id) + ": K must be >= 1";
  for (int round = 0; round < 1000; ++round) {
    if (set_error(-id, "thread %d: K must be >= %d", id, 1) != -id) ++thread_failures;
    if (round == 0) {  // both have written before either reads
      ++arrived;
      while (arrived.load() < 2) std::this_thread::yield();
    }
    if (mine != g_err.c_str()) ++thread_failures;
  }
  g_err.clear();
  if (g_err.c_str()[0] != '\0') ++thread_failures;
}

}  // namespace

int main() {
  static_assert(sizeof(ErrorState) == 512, "the buffer and nothing else");
  CHECK(g_err.c_str()[0] == '\0');  // starts empty

  // (a)
  CHECK(g_err.set(-10001, "%s: ld (%lld) < P (%lld)", "fedavg_reduce_f32", 5LL, 10LL) == -10001);
  CHECK(std::strcmp(g_err.c_str(), "fedavg_reduce_f32: ld (5) < P (10)") == 0);
  CHECK(set_error(7, "%s: launch failed: %s", "k", "why") == 7);
  CHECK(std::strcmp(g_err.c_str(), "k: launch failed: why") == 0);

  // (b) a heap copy, so that ASan sees a write one byte past the 512
  ErrorState* heap = new ErrorState;
  const std::string big(2000, 'x');
  CHECK(heap->set(3, "%s", big.c_str()) == 3);
  CHECK(std::strlen(heap->c_str()) == 511);
  CHECK(heap->text[511] == '\0');
  CHECK(std::string(heap->c_str()) == std::string(511, 'x'));
  CHECK(heap->set(4, "%s", std::string(511, 'y').c_str()) == 4);  // exactly fits
  CHECK(std::strlen(heap->c_str()) == 511);
  CHECK(heap->set(5, "%s", std::string(512, 'z').c_str()) == 5);  // one too many
  CHECK(std::strlen(heap->c_str()) == 511);
  delete heap;

  // (c)
  g_err.clear();
  CHECK(g_err.c_str()[0] == '\0' && std::strlen(g_err.c_str()) == 0);

  // (d)
  set_error(1, "main thread's message");
  std::thread a(worker, 1), b(worker, 2);
  a.join();
  b.join();
  CHECK(thread_failures.load() == 0);
  CHECK(std::strcmp(g_err.c_str(), "main thread's message") == 0);  // untouched by the workers

  std::printf("error_state_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
