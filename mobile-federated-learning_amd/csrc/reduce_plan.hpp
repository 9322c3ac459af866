// reduce_plan.hpp -- host arithmetic of the row reduce (fedavg_reduce_{f32,
// f64, f16, bf16}): the plan, the kernel forms a plan may name, and the
// round-split cut.  HIP-free on purpose, the device's CU count an argument:
// fedavg_reduce.hip includes it, and g++ compiles it with
// -fsanitize=address,undefined in tests/native/reduce_plan_check.cpp against
// the recorded plans of tests/reduce_plan_cases.txt.
//
// The production schedule was chosen from the in-process A/B sweeps in
// profiles/ (scripts/kernel_variants.py):
//   * column slices per thread C: the widest of 8/4/2/1 that still gives a
//     launch >= 512 blocks (a block then reads C*4 KiB contiguous bytes of
//     each client row per step); U (rows per load batch) = 4 for C = 8, else 8
//     (32 and 32/16/8 16-B loads in flight per thread);
//   * round-split dispatch: the column range is cut into the fewest equal
//     launches of <= 768 blocks (2-3 blocks per CU) -- one resident round
//     each, so every launch's blocks start together and sweep one compact
//     window of every row (88% of HBM peak at K=100 x P=25M vs 76% for one
//     multi-round launch of the same kernel);
//   * nontemporal loads (the rows are read once), except for working sets of
//     64-240 MiB, which stay resident in the 256 MiB Infinity Cache across
//     back-to-back rounds when loaded with the default policy (there U = 16,
//     C = 4 was fastest: 89% vs 81% for C = 1).
#pragma once

#include <cstdint>

#include "plan_table.hpp"

namespace fedavg_impl {

constexpr int kReduceBlock = 256;  // threads per workgroup of every planned form (common.hpp's kBlock)

// Round-split launches hold 3 blocks per CU (768 on the 256-CU MI355X); the
// CU count is the device's, so a partitioned GPU (fewer CUs per device) keeps
// one resident round per launch.
constexpr int kBlocksPerCU = 3;
constexpr int64_t kManyClients = 64;  // K from which the wider short-row schedules apply

// U rows per load batch x C 16-B slices per thread; nt: nontemporal loads;
// buf: per-row buffer descriptors (reduce_f32x4_buf_kernel /
// reduce_vec_buf_kernel, always nt); blocks_per_launch 0 = the resident
// blocks of the chosen instance
struct ReducePlan {
  int unroll, cols;
  bool nt, buf;
  int blocks_per_launch;
};

// The forms a plan may name, {U, C}; the only place they are written
// (fedavg_reduce.hip walks them, tests/product_kernels.txt lists the result).
constexpr PlanEntry kF32Nt[] = {{4, 8}, {8, 4}, {8, 2}, {8, 1}, {16, 4}, {16, 1}, {4, 6}, {8, 3}};
constexpr PlanEntry kF32Default[] = {{16, 4}};
constexpr PlanEntry kF32Buf[] = {{2, 16}, {8, 1}, {8, 2}};
constexpr PlanEntry kF64Nt[] = {{4, 8}, {8, 4}, {8, 2}, {8, 1}, {16, 4}, {16, 1}};
constexpr PlanEntry kF64Default[] = {{16, 4}};
constexpr PlanEntry kF64Buf[] = {{2, 16}};
constexpr PlanEntry kHalfNt[] = {{8, 4}, {4, 4}, {8, 2}, {8, 1}};
constexpr PlanEntry kHalfDefault[] = {{4, 4}};

// does the table of (lanes, p.nt, p.buf) hold {p.unroll, p.cols}
inline bool plan_has_form(int lanes, const ReducePlan& p) {
  const auto in = [&](const auto& table) {
    for (const PlanEntry& e : table)
      if (e.a == p.unroll && e.b == p.cols) return true;
    return false;
  };
  if (lanes == 4) return p.buf ? in(kF32Buf) : (p.nt ? in(kF32Nt) : in(kF32Default));
  if (lanes == 2) return p.buf ? in(kF64Buf) : (p.nt ? in(kF64Nt) : in(kF64Default));
  return !p.buf && (p.nt ? in(kHalfNt) : in(kHalfDefault));
}

// The instance production takes for K rows of P elements, row stride ld, of
// `lanes` elements per 16-B slice (4: fp32, 2: fp64, 8: fp16 / bf16) on a
// device of `cus` CUs.  The bands are the fp32 kernel's, measured in 16-B
// slices and bytes; fp64 / fp16 / bf16 take the fp32 problem with the same
// bytes per row (a 16-bit row's odd element does not count).
inline ReducePlan plan_reduce(int lanes, int64_t K, int64_t P, int64_t ld, int64_t cus) {
  const int64_t per4 = 16 / lanes;  // bytes per element
  const int64_t P4 = P * per4 / 4, ld4 = ld * per4 / 4;  // the row and its stride in 4-B units
  const int64_t nvec = (P4 + 3) / 4;
  const int64_t full = 2 * cus;  // blocks for a full-chip launch (512 on MI355X)
  const int round = kBlocksPerCU * static_cast<int>(cus);
  // a block's work is tiny (K rows): one launch, many short blocks; round
  // splitting would only add launch boundaries (K=2..3 sweeps: +14-22 %)
  if (K <= 4) return {8, 1, true, false, 1 << 30};

  // Infinity-Cache-resident band: default-policy loads, and a deep, wide
  // per-thread batch (16 rows x 4 slices) measured fastest there.  It applies
  // only when the whole row buffer the caller streams (K x ld) fits the band:
  // a chunk of a wider row buffer (ld > P) is not cache-resident between
  // calls: K=100 x 390K chunks of a 3.125M-column shard (the N=8 pipeline)
  // run 3,971 GB/s in the Infinity-Cache schedule and 5,065 streamed
  // (U16 x C1 nt; profiles/r01_chunk_rotating.jsonl)
  const double bytes = 4.0 * static_cast<double>(K) * static_cast<double>(P4);
  const double span_bytes = 4.0 * static_cast<double>(K) * static_cast<double>(ld4 > P4 ? ld4 : P4);
  const bool cached = bytes > 64.0 * (1 << 20) && span_bytes <= 240.0 * (1 << 20);
  // slices per thread by row length: 8, 4, 2, or 0 = short rows: few blocks,
  // so each thread's client chain is the critical path; deeper batches (16
  // rows) cut its round trips (+11-12 %), and with many clients 4 slices per
  // thread keep 64 loads in flight (`wide`)
  const int width = nvec >= full * kReduceBlock * 8 ? 8 : nvec >= full * kReduceBlock * 4 ? 4
                    : nvec >= full * kReduceBlock * 2 ? 2 : 0;
  const bool wide = nvec >= full / 4 * kReduceBlock * 4;

  if (lanes == 8) {
    // Each 16-B vector unpacks into 8 fp32 lanes of work, so the deep fp32
    // batches are cut to stay spill-free -- except the large-P form: there
    // the packed kernel wants the fp32 kernel's 32 x 16-B loads in flight per
    // thread as U8 x C4 (158 VGPRs), not U2 x C8 (16 loads): 6,543 vs 5,896
    // GB/s at K=100 x P=25M bf16 and 6,641 vs 6,595 at K=500 x P=11.2M
    // (profiles/sweeps/r01_half_*.jsonl).
    if (cached) return {4, 4, false, false, round};
    if (width == 8) return {8, 4, true, false, round};
    if (width == 4) return {4, 4, true, false, round};
    if (width == 2) return {8, 2, true, false, round};
    return K >= 500 && wide ? ReducePlan{4, 4, true, false, round} : ReducePlan{8, 1, true, false, round};
  }

  if (lanes == 4 && K < kManyClients && width < 8) {
    // Few clients (5 <= K < 64) on rows below the 8-slice band: per-row buffer
    // descriptors with 1-2 slices per thread and a launch of every resident
    // block.  rocprofv3 kernel time, variants interleaved in one process, two
    // sweeps (scripts/buf_probe.py; profiles/r02/sweeps/small_k_*.json):
    //   4-slice band (2.1M <= P < 4.2M): U8 x C2 -- K=5 x 2.4M 0.68-0.73 x the
    //     time of U8 x C4 (nt), K=10 x 2.4M 0.72-0.73 x U16 x C4 (Infinity-Cache
    //     band), K=32 / 50 x 2.4M 0.89 / 0.94 x;
    //   shorter rows, 8 <= K <= 32, P >= 262K: U8 x C1 -- K=10 x 1.2M (FEMNIST)
    //     0.88 x, K=10 x 300K 0.69-0.73 x, K=20 / 32 x 1.2M 0.81-0.85 / 0.73 x,
    //     K=32 x 300K 0.80 x; K=5 and K=50 gain nothing there.
    // (K >= 64 keeps the rules below, tuned on the all-gather chunk shapes.)
    if (width == 4) return {8, 2, true, true, 0};
    if (K >= 8 && K <= 32 && nvec >= full * kReduceBlock / 2) return {8, 1, true, true, 0};
  }
  if (cached) return {16, 4, false, false, round};
  // Rows long enough for a full-chip launch (2 blocks per CU) of 16-slice
  // groups take U2 x C16 through per-row buffer descriptors (32-bit lane
  // offsets shared by every row): fp32 7.09-7.15 vs 6.96-7.05 TB/s at K=100 x
  // 25M and 6.89 vs 6.49 at K=100 x 10M, interleaved (scripts/buf_probe.py,
  // profiles/r01_buf_probe*.jsonl); below that width the 16-slice groups
  // leave the launch short of blocks (4.4 TB/s at K=100 x 5M).  fp64 follows:
  // 7,113 vs 6,992 GB/s at K=100 x 12.5M fp64 (scripts/vec_buf_probe.py,
  // profiles/r01_vec_buf_probe.jsonl).  fp16/bf16 measured no gain (+0-1 %).
  if (nvec >= full * kReduceBlock * 16) return {2, 16, true, true, round};
  if (width == 8) return {4, 8, true, false, round};

  if (lanes == 4 && K >= kManyClients) {
    // short rows with many clients (the N > 1 all-gather chunks): 4 slices per
    // thread -- K=100 x 1.56M (N=2 chunk) 6,695 vs 6,178 GB/s at U8 x C2, and
    // K=100 x 781K (N=4 chunk) 6,741 vs 5,668 at U16 x C1
    // (profiles/r01_chunk_shapes.jsonl, interleaved)
    // Rows that give 3/4 to 1 block per CU at 6 (K >= 64) or 3 (K >= 256)
    // slices per thread: one resident block on (nearly) every CU beats
    // 1.5 blocks per CU at 4 slices.  Rotating-chunk sweep, interleaved,
    // bit-identical (profiles/r02/sweeps/short_row_c3_c6.jsonl): K=100 x 1.56M
    // (the N=2 chunk) 6,822 vs 6,585 GB/s at U8 x C4; K=500 x 702K (cfg4's
    // N=8 chunk) 6,856 vs 6,627 at U16 x C4.  (K=100 x 781K keeps U16 x C4:
    // 6,527 vs 6,200 at C3.)
    if (nvec >= cus * 3 / 4 * kReduceBlock * 6 && nvec <= cus * kReduceBlock * 6) return {4, 6, true, false, round};
    if (K >= 256 && nvec >= cus * 3 / 4 * kReduceBlock * 3 && nvec <= cus * kReduceBlock * 3)
      return {8, 3, true, false, round};
    if (width >= 2) return {8, 4, true, false, round};
    return {16, wide ? 4 : 1, true, false, round};
  }
  if (width >= 2) return {8, width, true, false, round};
  return {16, K >= 500 && wide ? 4 : 1, true, false, round};
}

// Round-split dispatch: the column range (nvec 16-B slices, `span` per
// block) is cut into the fewest EQUAL launches whose blocks all fit on the
// chip at once (one resident round of `resident` blocks each).  Within a
// launch every block starts together and the running blocks sweep one compact
// window of every client row; the stream boundary between launches re-aligns
// them (a multi-round launch lets blocks drift apart and leaves a half-empty
// last round).  The one statement of the cut: slices per launch, a multiple
// of span, and the launches that covers nvec with.
struct RoundSplit {
  int64_t per;
  int launches;
};

inline RoundSplit round_split(int64_t nvec, int64_t span, int64_t resident) {
  if (nvec <= 0) return {span, 0};
  const int64_t blocks = (nvec + span - 1) / span;
  const int64_t nl = (blocks + resident - 1) / resident;
  const int64_t per = ((nvec + nl - 1) / nl + span - 1) / span * span;
  return {per, static_cast<int>((nvec + per - 1) / per)};
}

// f(v0, n, tail, first, last) per launch, in order: slices [v0, v0 + n);
// `tail` (the valid lanes of the row's last slice, 0 = all) goes to the last
// launch only
template <class F>
void for_each_launch(const RoundSplit& rs, int64_t nvec, int tail, F&& f) {
  for (int64_t v0 = 0; v0 < nvec; v0 += rs.per) {
    const int64_t n = (nvec - v0) < rs.per ? (nvec - v0) : rs.per;
    const bool last = v0 + n == nvec;
    f(v0, n, last ? tail : 0, v0 == 0, last);
  }
}

}  // namespace fedavg_impl
