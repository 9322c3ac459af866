// The [K, ld] rows passes' host arithmetic (csrc/dist_plan.hpp) under
// sanitizers (test infrastructure; no GPU).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       -I mobile-federated-learning_amd/csrc tests/native/dist_plan_check.cpp -o /tmp/dist_plan_check
//   /tmp/dist_plan_check tests/dist_plan_cases.txt     (tests/test_native_sanitized.py runs it)
//
// The fixture was recorded from the planner text fedavg_dist.hip held before
// this header existed, with fixed tables of resident workgroups per kernel
// instance in place of the occupancy queries; its `stub` lines state those
// tables and stub_parts() below answers from them.  What is checked:
// (a) fused_plan, fused_workspace, dist_plan, dist_workspace, dist_vec_plan
//     and dist_vec_workspace equal every recorded line -- every K and P of the
//     GPU geometry test, P at +-1 around every residency-dependent edge, under
//     a 256-CU and a 64-CU stub;
// (b) every plan names an entry of its table (kWinBands / kSplitForms /
//     kLdsTiles / kRsTiles / kDistBufForms / kDistVecForms): the walks in
//     fedavg_dist.hip return FEDAVG_EMODE otherwise;
// (c) the fused workspace is never below K x parts of the chosen plan, nor
//     below the two passes' size;
// (d) every register-staged plan's slots cover its K, and every tile plan's
//     LDS bytes are <= 160 KiB at the largest K of its band;
// (e) round_split(nvec, span, cap) / for_each_launch give the nl and
//     per_blocks of the hand-written loop they replaced in launch_sqdist (the
//     H digests over every nvec 1..5 x span x cap), the launches tile
//     [0, nvec) in order, and the tail goes to the last launch only.
// Exit status 0 = clean; any finding aborts (ASan/UBSan) or returns 1.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <utility>

#include "dist_plan.hpp"

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

// a stub residency table (the fixture's `stub` lines)
struct Stub {
  int64_t cus = 0, lds = 0, split8 = 0, split16 = 0, slots16 = 0, slots8 = 0;
  std::map<int, int64_t> win, ldscap;            // KMAX / S -> workgroups per CU
  std::map<std::pair<int, int>, int64_t> rscap;  // {S, slots} -> workgroups per CU
};

template <size_t N>
bool in_table(const PlanEntry (&t)[N], int a, int b = kAnyB) {
  for (const PlanEntry& e : t)
    if (e.a == a && (b == kAnyB || e.b == b)) return true;
  return false;
}

// the table entry a fused plan names (with_fused_instance's walk)
bool plan_has_instance(const FusedPlan& p) {
  switch (p.kind) {
    case kFusedWin: return in_table(kWinBands, p.S);
    case kFusedWinn: return in_table(kSplitForms, p.slots <= 8 ? 8 : 16);
    case kFusedLds: return in_table(kLdsTiles, p.S);
    case kFusedRs: return in_table(kRsTiles, p.S, p.slots);
  }
  return false;
}

// parts(plan, K, P) as the instance tags answer it, from the stub
int64_t stub_parts(const Stub& st, const FusedPlan& p, int64_t K, int64_t P) {
  if (!plan_has_instance(p)) return 0;
  const auto lds_per_cu = [&](int64_t cap, int64_t bytes) { return bytes > st.lds ? 0 : std::min(cap, st.lds / bytes); };
  switch (p.kind) {
    case kFusedWin: {
      const int vec = win_band_of(p.S)->b;
      return window_waves(std::max<int64_t>(st.win.at(p.S), 1), st.cus, (P + 64 * vec - 1) / (64 * vec), 4);
    }
    case kFusedWinn: {
      const int64_t per_cu = (p.slots <= 8 ? st.split8 : st.split16) / ((K + 63) / 64);
      return persistent_grid(split_per_cu(std::max<int64_t>(per_cu, 1) * st.cus, st.cus), st.cus, (P + 63) / 64);
    }
    case kFusedLds:
      return persistent_grid(lds_per_cu(st.ldscap.at(p.S), fused_lds_bytes(K, p.S)), st.cus, (P + p.S - 1) / p.S);
    default:
      return persistent_grid(lds_per_cu(st.rscap.at({p.S, p.slots}), fused_rs_lds_bytes(K, p.S)), st.cus,
                             (P + p.S - 1) / p.S);
  }
}

// (e) one cut against the replaced loop's nl / per_blocks, and the launches' coverage
void check_cut(int64_t nvec, int64_t span, int64_t cap, int tail, const RoundSplit& rs) {
  const int64_t blocks = (nvec + span - 1) / span;
  const int64_t nl = (blocks + cap - 1) / cap;
  const int64_t per_blocks = (blocks + nl - 1) / nl;
  CHECK(rs.launches == nl && rs.per == per_blocks * span, "nvec %" PRId64 " span %" PRId64 " cap %" PRId64, nvec, span,
        cap);
  int64_t next = 0, n_launches = 0;
  for_each_launch(rs, nvec, tail, [&](int64_t v0, int64_t n, int t, bool first, bool last) {
    CHECK(v0 == next && v0 % span == 0 && n > 0 && (n + span - 1) / span <= cap && t == (last ? tail : 0) &&
              first == (v0 == 0),
          "launch at %" PRId64 " of %" PRId64 " slices", v0, n);
    next = v0 + n;
    ++n_launches;
  });
  CHECK(next == nvec && n_launches == nl, "launches end at %" PRId64 " of %" PRId64, next, nvec);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: %s tests/dist_plan_cases.txt\n", argv[0]);
    return 2;
  }
  std::ifstream f(argv[1]);
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::map<std::string, Stub> stubs;
  int cases = 0, digests = 0;
  std::string line, tag, name, field, arrow;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    in >> tag >> name;
    if (tag == "stub") {
      Stub& st = stubs[name];
      in >> field;
      if (field == "cus")
        in >> st.cus >> field >> st.lds >> field >> st.split8 >> field >> st.split16 >> field >> st.slots16 >> field >>
            st.slots8;
      if (field == "win")
        for (int kmax; in >> kmax;) in >> st.win[kmax];
      if (field == "ldscap")
        for (int s; in >> s;) in >> st.ldscap[s];
      if (field == "rscap")
        for (int s, slots; in >> s >> slots;) in >> st.rscap[{s, slots}];
      continue;
    }
    ++cases;
    if (tag == "H") {
      const int C = std::stoi(name);
      int64_t cap, n;
      uint64_t want, h = 1469598103934665603ull;
      in >> cap >> n >> arrow >> want;
      const int64_t span = static_cast<int64_t>(kReduceBlock) * C;
      CHECK(n == 5 * span * cap, "digest over %" PRId64 " slice counts", n);
      const auto mix = [&](int64_t v) {
        for (int i = 0; i < 8; ++i) h = (h ^ ((uint64_t(v) >> (8 * i)) & 0xff)) * 1099511628211ull;
      };
      for (int64_t nvec = 1; nvec <= n; ++nvec) {
        const RoundSplit rs = round_split(nvec, span, cap);
        mix(rs.launches);
        mix(rs.per / span);
        // the launches themselves at every count up to two full launches, then at a stride and at the block edges
        if (nvec <= 2 * span * cap || nvec % 997 == 0 || nvec % span <= 1) check_cut(nvec, span, cap, int(nvec & 3), rs);
      }
      CHECK(h == want, "round_split digest at C %d cap %" PRId64, C, cap);
      ++digests;
      continue;
    }
    const Stub& st = stubs.at(name);
    const auto parts = [&](const FusedPlan& p, int64_t K, int64_t P) { return stub_parts(st, p, K, P); };
    if (tag == "F") {
      int64_t K, P, want_parts, want_ws;
      int kind, S, slots;
      in >> K >> P >> arrow >> kind >> S >> slots >> want_parts >> want_ws;
      const FusedPlan p = fused_plan(K, P, parts);
      const int64_t two_pass = dist_workspace(K, P, dist_plan(P, st.cus, st.slots16, st.slots8));
      const int64_t ws = fused_workspace(K, P, two_pass, parts);
      CHECK(p.kind == kind && p.S == S && p.slots == slots && parts(p, K, P) == want_parts && ws == want_ws,
            "%s K %" PRId64 " P %" PRId64 ": plan %d %d %d parts %" PRId64 " ws %" PRId64 ", recorded %d %d %d %" PRId64
            " %" PRId64, name.c_str(), K, P, p.kind, p.S, p.slots, parts(p, K, P), ws, kind, S, slots, want_parts, want_ws);
      CHECK(p.kind == kFusedNone ? K > kFusedRowsMaxK : plan_has_instance(p), "plan %d / %d / %d names no entry", p.kind,
            p.S, p.slots);                                                              // (b)
      CHECK(ws >= K * parts(p, K, P) && ws >= two_pass, "workspace %" PRId64, ws);      // (c)
      if (p.kind == kFusedRs) CHECK(fused_rs_slots_cover(K, p.S, p.slots), "slots at K %" PRId64, K);  // (d)
    } else if (tag == "D") {
      int64_t K, P, want_ws;
      int U, C;
      in >> K >> P >> arrow >> U >> C >> want_ws;
      const PlanEntry p = dist_plan(P, st.cus, st.slots16, st.slots8);
      CHECK(p.a == U && p.b == C && dist_workspace(K, P, p) == want_ws, "%s K %" PRId64 " P %" PRId64 ": U%d x C%d",
            name.c_str(), K, P, p.a, p.b);
      CHECK(in_table(kDistBufForms, p.a, p.b) && dist_chains(p.b) >= 1 && dist_chains(p.b) <= p.b, "form U%d x C%d", p.a,
            p.b);
    } else if (tag == "V") {
      int64_t es, K, P, want_ws;
      int U, C;
      in >> es >> K >> P >> arrow >> U >> C >> want_ws;
      const PlanEntry p = dist_vec_plan(dist_vec_slices(P, es), st.cus);
      CHECK(p.a == U && p.b == C && dist_vec_workspace(K, P, es, st.cus) == want_ws,
            "%s es %" PRId64 " K %" PRId64 " P %" PRId64 ": U%d x C%d", name.c_str(), es, K, P, p.a, p.b);
      CHECK(in_table(kDistVecForms, p.a, p.b), "form U%d x C%d", p.a, p.b);
    } else {
      std::fprintf(stderr, "bad fixture line: %s\n", line.c_str());
      return 2;
    }
    CHECK(!in.fail(), "short fixture line: %s", line.c_str());
  }
  // (d) LDS bytes at the largest K of each tile band (fused_plan's K edges)
  constexpr int64_t kLdsMax = 160 * 1024;
  CHECK(fused_rs_lds_bytes(16, 256) <= kLdsMax && fused_lds_bytes(32, 128) <= kLdsMax &&
            fused_lds_bytes(48, 256) <= kLdsMax && fused_lds_bytes(64, 128) <= kLdsMax &&
            fused_lds_bytes(128, 64) <= kLdsMax && fused_rs_lds_bytes(192, 64) <= kLdsMax &&
            fused_rs_lds_bytes(320, 32) <= kLdsMax && fused_rs_lds_bytes(kFusedWinnMinK - 1, 32) <= kLdsMax,
        "a tile band's LDS bytes exceed 160 KiB");
  CHECK(dist_workspace(0, 5, kDistBufForms[0]) == 0 && dist_vec_workspace(3, 5, 3, 256) == 0 &&
            dist_vec_workspace(0, 5, 4, 256) == 0 && dist_vec_workspace(3, 0, 4, 256) == 0,
        "empty shapes need no workspace");
  CHECK(cases > 1200 && stubs.size() == 2 && digests == 25 && stubs.count("mi355x") && stubs.at("mi355x").cus == 256 &&
            stubs.at("small").cus == 64,
        "fixture: %d cases, %zu stubs, %d digests", cases, stubs.size(), digests);
  std::printf("%d fixture cases, %lld checks, %d failures\n", cases, checks, failures);
  return failures ? 1 : 0;
}
