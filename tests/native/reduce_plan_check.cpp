// The row reduce's host arithmetic (csrc/reduce_plan.hpp) under sanitizers
// (test infrastructure; no GPU).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I mobile-federated-learning_amd/csrc tests/native/reduce_plan_check.cpp -o /tmp/reduce_plan_check
//   /tmp/reduce_plan_check tests/reduce_plan_cases.txt [seed]     (tests/test_native_sanitized.py runs it)
//
// What it checks, with the device's CU count fixed at 256 as in the fixture:
// (a) plan_reduce equals every line of the fixture (the plans recorded from
//     the planner this header replaced);
// (b) every plan of the fixture's sweep, and of 100,000 seeded random
//     (lanes, K <= 2048, P <= 2^31, ld >= P) draws on several CU counts, has
//     an entry in its dtype's form table -- the walk in fedavg_reduce.hip
//     returns FEDAVG_EMODE otherwise, so this is what makes that unreachable;
// (c) round_split / for_each_launch, for every plan of the sweep at resident
//     in {1, 3, 768, 1024, 2^30} and at the plan's own blocks_per_launch (the
//     first 2,000 random draws too, at 768 and up): the launches tile
//     [0, nvec) exactly once and in order, each holds <= resident blocks,
//     every cut but the last is a multiple of span, only the last launch
//     carries the tail, exactly one launch is first and one last, and
//     `launches` is the number of iterations;
// (d) `launches` equals ceil(blocks / resident), the formula the schedule
//     entry points used to report.
// Exit status 0 = clean; any finding aborts (ASan/UBSan) or returns 1.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "reduce_plan.hpp"

using namespace fedavg_impl;

namespace {

int failures = 0;
long long checks = 0;
#define CHECK(cond, ...)                                        \
  do {                                                          \
    ++checks;                                                   \
    if (!(cond)) {                                              \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);                        \
      std::fprintf(stderr, "\n");                               \
      if (++failures > 20) std::exit(1);                        \
    }                                                           \
  } while (0)

constexpr int64_t kResidents[] = {1, 3, 768, 1024, int64_t(1) << 30};

// (c) and (d) for one cut
void check_split(int lanes, int64_t P, int cols, int64_t resident) {
  const int64_t nvec = (P + lanes - 1) / lanes, span = int64_t(kReduceBlock) * cols;
  const int tail = static_cast<int>(P % lanes);
  const RoundSplit rs = round_split(nvec, span, resident);
  int64_t next = 0;
  int iterations = 0, firsts = 0, lasts = 0;
  for_each_launch(rs, nvec, tail, [&](int64_t v0, int64_t n, int t, bool first, bool last) {
    CHECK(v0 == next && n > 0, "launch %d starts at %" PRId64 ", expected %" PRId64, iterations, v0, next);
    CHECK((n + span - 1) / span <= resident, "launch of %" PRId64 " slices > %" PRId64 " blocks of %" PRId64, n, resident,
          span);
    CHECK(last == (v0 + n == nvec) && first == (v0 == 0), "first/last flags at %" PRId64, v0);
    CHECK(last || (v0 + n) % span == 0, "cut at %" PRId64 " is no multiple of span %" PRId64, v0 + n, span);
    CHECK(t == (last ? tail : 0), "tail %d in launch %d (last %d)", t, iterations, int(last));
    next = v0 + n;
    ++iterations, firsts += first, lasts += last;
  });
  CHECK(next == nvec && firsts == 1 && lasts == 1, "coverage ends at %" PRId64 " of %" PRId64, next, nvec);
  CHECK(rs.launches == iterations, "launches %d != %d iterations", rs.launches, iterations);
  const int64_t blocks = (nvec + span - 1) / span;
  CHECK(rs.launches == (blocks + resident - 1) / resident,
        "launches %d != ceil(%" PRId64 " blocks / %" PRId64 ") (lanes %d P %" PRId64 " cols %d)", rs.launches, blocks,
        resident, lanes, P, cols);
}

// splits at every resident >= min_resident (0: none; a long random row at 1 block per launch is millions of launches)
void check_plan(int lanes, int64_t K, int64_t P, int64_t ld, int64_t cus, int64_t min_resident) {
  const ReducePlan p = plan_reduce(lanes, K, P, ld, cus);
  CHECK(plan_has_form(lanes, p),
        "no table entry: lanes %d K %" PRId64 " P %" PRId64 " ld %" PRId64 " cus %" PRId64 " -> U%d C%d nt%d buf%d", lanes,
        K, P, ld, cus, p.unroll, p.cols, int(p.nt), int(p.buf));
  CHECK(p.blocks_per_launch >= 0 && (p.blocks_per_launch > 0 || p.buf), "blocks_per_launch %d", p.blocks_per_launch);
  if (!min_resident) return;
  for (int64_t r : kResidents)
    if (r >= min_resident) check_split(lanes, P, p.cols, r);
  if (p.blocks_per_launch > 0) check_split(lanes, P, p.cols, p.blocks_per_launch);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s tests/reduce_plan_cases.txt [seed]\n", argv[0]);
    return 2;
  }
  const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1234;
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  char line[256];
  int cases = 0;
  while (std::fgets(line, sizeof(line), f)) {
    if (line[0] == '#' || line[0] == '\n') continue;
    int lanes, U, C, nt, buf, bpl;
    int64_t K, P, ld;
    if (std::sscanf(line, "%d %" SCNd64 " %" SCNd64 " %" SCNd64 " -> %d %d %d %d %d", &lanes, &K, &P, &ld, &U, &C, &nt, &buf,
                    &bpl) != 9) {
      std::fprintf(stderr, "bad fixture line: %s", line);
      return 2;
    }
    ++cases;
    const ReducePlan p = plan_reduce(lanes, K, P, ld, 256);
    CHECK(p.unroll == U && p.cols == C && p.nt == (nt != 0) && p.buf == (buf != 0) && p.blocks_per_launch == bpl,
          "lanes %d K %" PRId64 " P %" PRId64 " ld %" PRId64 ": fixture U%d C%d nt%d buf%d bpl%d, plan U%d C%d nt%d buf%d bpl%d",
          lanes, K, P, ld, U, C, nt, buf, bpl, p.unroll, p.cols, int(p.nt), int(p.buf), p.blocks_per_launch);
    check_plan(lanes, K, P, ld, 256, 1);
  }
  std::fclose(f);
  CHECK(cases > 0, "empty fixture");

  std::mt19937_64 rng(seed);
  const int64_t cu_counts[] = {256, 256, 256, 304, 128, 64, 32, 8, 1};
  for (int i = 0; i < 100000; ++i) {
    const int lanes = 2 << (rng() % 3);  // 2, 4, 8
    const int64_t K = 1 + static_cast<int64_t>(rng() % 2048);
    // half the draws small enough to meet the short-row bands
    const int64_t P = 1 + static_cast<int64_t>(rng() % ((i & 1) ? (uint64_t(1) << 31) : (uint64_t(1) << 24)));
    const int64_t ld = P + static_cast<int64_t>(rng() % 3 == 0 ? 0 : rng() % (2 * static_cast<uint64_t>(P) + 1));
    check_plan(lanes, K, P, ld, cu_counts[rng() % 9], i < 2000 ? 768 : 0);
  }
  std::printf("%d fixture cases, 100000 random plans, %lld checks, %d failures\n", cases, checks, failures);
  return failures ? 1 : 0;
}
