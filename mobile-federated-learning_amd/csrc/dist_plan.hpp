// dist_plan.hpp -- host arithmetic of the [K, ld] rows passes of fedavg_dist.hip: the fused
// aggregate + :291 pass's plan (fedavg_reduce_sqdist_f32) and the distance pass's
// (fedavg_client_sqdist_{f32, f64, f16, bf16}), their form tables, LDS sizes and workspace
// bounds.  HIP-free on purpose, as reduce_plan.hpp and segments_plan.hpp: the CU count is an
// argument and the kernels' residency a callable or a number.  fedavg_dist.hip passes its
// instance tags' occupancy queries, tests/native/dist_plan_check.cpp (g++, ASan + UBSan) a
// fixed table, against tests/dist_plan_cases.txt.
#pragma once

#include <cstdint>

#include "plan_table.hpp"
#include "reduce_plan.hpp"

namespace fedavg_impl {

// ---------------------------------------------------------------------------
// The fused pass (aggregate + :291 in one read of the rows)
// ---------------------------------------------------------------------------
// Which one-read kernel serves K rows (production), from interleaved
// measurements of every candidate against the others and the two passes on
// ~4 GB of rows (scripts/fused_probe.py, profiles/r03/fused_rule/*.jsonl and
// profiles/r03/win/*.jsonl; ms):
//   long rows (>= 16 windows per wave), 17 <= K <= 128: the wave-owned
//   windows (reduce_sqdist_win_kernel), KMAX x VEC by K:
//     K <= 48   48 x 4 (1 KiB per wave per row; 24 x 41.7M 0.675 vs 0.697
//               LDS-DMA 128 and 0.687 at 32 x 4; 32 x 31.3M 0.715 vs 0.736;
//               48 x 20.8M 0.652 vs 0.687 LDS-DMA 256)
//     K <= 64   64 x 2 (64 x 10M 0.449 vs 0.464; 56 x 20M 0.841 vs 0.867)
//     K <= 80   80 x 2 (72 x 25M 1.311 vs 1.915 LDS-DMA 64; 80 x 25M 1.397
//               vs 2.124 -- the LDS-DMA tiles at 65-90 rows run far below
//               their K = 100 rate)
//     K <= 100  100 x 2 (100 x 25M 1.531-1.665 vs 1.601-1.797 by box; 90 x
//               25M 1.578 vs 2.440; 100 x 6.25M 0.431 vs 0.451)
//     K <= 128  128 x 1 (128 x 8M 0.693 vs 0.879; 112 x 8M 0.610 vs 0.640)
//   shorter rows (100 x 3.1M: window 0.230 vs 0.218; 65-96 rows from 400K
//   columns up stay on the windows, see kWinHoleMinP), other K:
//   K <= 16    register-staged, 256-column tiles (8 x 125M 0.896 vs 0.880
//              LDS-DMA; FEMNIST 10 x 1.2M 16.6 vs 22.2 us)
//   K <= 32    LDS-DMA, 128 columns (24 x 41.7M 0.733 vs 0.738 register-staged)
//   K <= 48    LDS-DMA, 256 columns (48 x 20.8M 0.737 vs 0.758 at 128)
//   K <= 64    LDS-DMA, 128 columns (64 x 10M 0.472 vs 0.486 register-staged)
//   K <= 128   LDS-DMA, 64 columns (100 x 25M 1.654 vs 1.753 register-staged)
//   K <= 192   register-staged, 64 columns, 16 slots (192 x 5.2M 0.778 vs
//              0.857 at 32 columns; the LDS-DMA kernel 0.829)
//   K <= 320   register-staged, 32 columns, 10 slots (224 x 4.5M 0.728 vs
//              1.03 at 64; 300 x 5M 1.08 vs 1.41 LDS-DMA vs 1.98 two passes)
//   K <= 368   register-staged, 32 columns, 16 slots (round 3: 500 x 11.2M
//              5.41 vs 6.88 ms for the two passes; 512 x 5M 2.58 vs 3.22)
//   K <= 1024  split-row windows (round 5, below: kFusedWinnMinK)
// Beyond 1024 rows the two passes (a workgroup holds at most 16 x 64 rows).
constexpr int kFusedNone = 0, kFusedLds = 1, kFusedRs = 2, kFusedWin = 3, kFusedWinn = 4;
constexpr int64_t kFusedRowsMaxK = 1024;
// split-row windows (64 rows per wave, 64 columns) from 369 rows (round 5's
// barrier form, since retired; scripts/fused_probe.py, profiles/r05/winn/, ms:
// 384 x 5M 1.455 vs 1.494 register-staged; 448 x 5M 1.60 vs 2.30; 500 x
// 11.2M 3.71 vs 5.37; 500 x 1.4M 0.54 vs 0.72; 512 x 5M 1.69 vs 2.59; but
// 352 x 5M 1.42 vs 1.36 and 300 x 5M 1.10 vs 1.05), up to 8 waves per
// workgroup to 512 rows, 16 beyond (640 x 3M 1.77 vs 2.46 for the two
// passes; 1000 x 12.5M 9.99 vs 15.05; 520 x 5M 2.71 vs 3.34)
constexpr int64_t kFusedWinnMinK = 369;
// Round 6: the split windows run reduce_sqdist_winf_kernel (point-to-point
// hand-offs, broadcast weights) with 8 prefetched rows at <= 8 waves and 16
// beyond (profiles/r06/winf/, ms, barrier form vs winf: 1000 x 12.5M 9.06 vs
// 8.02; 999 x 10M+3 7.75 vs 6.44; 600 x 10M 5.13 vs 4.28; 513 x 3M 1.48 vs
// 1.26; 500 x 11.2M 3.66 vs 3.57; 400 x 10M 2.73 vs 2.60; 370 x 5M 1.25 vs
// 1.18; every output bit-identical).
// (kSplitForms, plan_table.hpp: for_split gives <8, PF 8> or <16, PF 16>)
// With the prefetch the split windows also beat the register-staged tiles at
// 161-256 and 289-368 rows on long rows (profiles/r05/prefetch/, ms, tiles vs
// split: 170 x 5M 0.606 vs 0.593; 192 x 5M 0.725 vs 0.661; 240 x 5M 0.897 vs
// 0.822; 256 x 12M 2.53 vs 2.19; 290 x 5M 1.026 vs 0.998; 310 x 5M 1.092 vs
// 1.033; 352 x 5M 1.347 vs 1.178; 368 x 5M 1.427 vs 1.228), not at 140 x 5M
// (0.493 vs 0.529) or 270 x 5M (0.933 vs 0.981), and tie at 200 x 1.2M (18
// windows per workgroup): below 369 rows they took rounds of >= 24 windows
// per workgroup
// Round 6, the hand-off kernel (profiles/r06/winf_bands/, ms, plan then vs
// winf): 160 x 5M 0.615 vs 0.547; 260 x 5M 0.913 vs 0.851; 270 x 5M 0.939 vs
// 0.876; 288 x 5M 0.983 vs 0.923 (the old 257-288 gap); 200 x 1.2M (18
// windows per workgroup) 0.190 vs 0.182; 200 x 800K (12) 0.144 vs 0.126;
// 300-368 x 5M equal; below 160 the tiles keep it (150 x 5M 0.526 vs 0.536,
// 130 x 5M 0.459 vs 0.495)
constexpr int64_t kFusedWinnLowMinK = 160;
constexpr int64_t kFusedWinnLowMinPerBlock = 8;
constexpr int64_t kWinMinPerWave = 16;  // windows per wave below which the tile kernels keep the round
// ... except in the LDS-DMA tiles' weak band, 65-96 rows, where the windows
// win down to ~400K columns (profiles/r03/win/short_rows_*.jsonl, ms, tiles
// vs windows: 70 x 600K 0.052 vs 0.043; 70 x 3M 0.217 vs 0.143; 80 x 1.5M
// 0.129 vs 0.090; 90 x 600K 0.065 vs 0.051; 90 x 3M 0.285 vs 0.190; 92 x
// 1.5M 0.108 vs 0.102; 98 x 1.5M 0.109 vs 0.109; 100 x 600K 0.059 vs 0.059;
// 65 x 200K 0.022 vs 0.023)
constexpr int64_t kWinHoleMinK = 65, kWinHoleMaxK = 96, kWinHoleMinP = 400000;
struct FusedPlan {
  int kind, S, slots;  // kFusedWin: S = KMAX, slots = VEC
};

// The 81-100 band stages rows 0..23 of the next window in LDS (MODE 64):
// 100 x 25M 1.652 -> 1.646 ms, 100 x 25M+3 1.700 -> 1.690, 90 x 25M 1.607 ->
// 1.547 (profiles/r03/win/ldsrows.jsonl); every band has K > 24 rows
constexpr int kWin100Mode = 64;

constexpr int win_rows_mode(int kmax) { return kmax == 100 ? kWin100Mode : 0; }

// the window kernel instance for K rows ({kFusedNone} outside 17..128: kWinBands, plan_table.hpp)
inline FusedPlan win_plan(int64_t K) {
  const PlanEntry* band = win_band_of(K);
  return band ? FusedPlan{kFusedWin, band->a, band->b} : FusedPlan{kFusedNone, 0, 0};
}

// The tile plans' instances: LDS-DMA tiles by columns, register-staged tiles
// by {columns, slots}.  fused_plan returns entries of these tables.
constexpr PlanEntry kLdsTiles[] = {{64, 0}, {128, 0}, {256, 0}};
constexpr PlanEntry kRsTiles[] = {{256, 8}, {64, 16}, {32, 10}, {32, 16}};

// LDS of an LDS-DMA tile:
// the tile + its average, and at least the 256 doubles of the final per-row sums
inline int64_t fused_lds_bytes(int64_t K, int S, bool db = false) {
  const int64_t b = ((db ? 2 : 1) * K + 1) * S * 4;
  return b > kReduceBlock * 8 ? b : kReduceBlock * 8;
}
// LDS of a register-staged tile: [K][S] + the average [S]; the final per-row
// sums need K * V doubles (= K * S * 2 bytes, inside the tile)
inline int64_t fused_rs_lds_bytes(int64_t K, int S) { return (K + 1) * S * 4; }
// a register-staged tile's K x S / 4 slices fit `slots` 16-B slots of each of the 256 threads
constexpr bool fused_rs_slots_cover(int64_t K, int S, int slots) { return (K * S + 1023) / 1024 <= slots; }

// The production plan of K rows of P columns.  parts(plan, K, P) = the
// partials' second dimension of that plan's production launch (workgroups;
// one-wave windows: waves), 0 when the plan names no instance or it is not
// resident -- seg_fused_plan's convention (segments_plan.hpp).
template <class Parts>
FusedPlan fused_plan(int64_t K, int64_t P, Parts&& parts) {
  if (K < 1 || K > kFusedRowsMaxK) return {kFusedNone, 0, 0};
  const FusedPlan win = win_plan(K);
  if (win.kind == kFusedWin && ((P + 64 * win.slots - 1) / (64 * win.slots) >= kWinMinPerWave * parts(win, K, P) ||
                                 (K >= kWinHoleMinK && K <= kWinHoleMaxK && P >= kWinHoleMinP)))
    return win;
  if (K <= 16) return {kFusedRs, 256, 8};
  if (K <= 32) return {kFusedLds, 128, 0};
  if (K <= 48) return {kFusedLds, 256, 0};
  if (K <= 64) return {kFusedLds, 128, 0};
  if (K <= 128) return {kFusedLds, 64, 0};
  if (K >= kFusedWinnLowMinK && K < kFusedWinnMinK) {
    const int64_t grid = parts(FusedPlan{kFusedWinn, 64, 8}, K, P);
    if (grid > 0 && (P + 63) / 64 >= kFusedWinnLowMinPerBlock * grid) return {kFusedWinn, 64, 8};
  }
  if (K <= 192) return {kFusedRs, 64, 16};
  if (K <= 320) return {kFusedRs, 32, 10};
  if (K < kFusedWinnMinK) return {kFusedRs, 32, 16};
  return {kFusedWinn, 64, K <= 512 ? 8 : 16};  // S = rows per wave, slots = waves per workgroup (max)
}

// fedavg_reduce_sqdist_workspace: the fused launch's K x parts, never below
// the two passes' bound (`two_pass`: dist_workspace), which serve unaligned
// out / weights and K > kFusedRowsMaxK
template <class Parts>
int64_t fused_workspace(int64_t K, int64_t P, int64_t two_pass, Parts&& parts) {
  const int64_t fused = K * parts(fused_plan(K, P, parts), K, P);
  return fused > two_pass ? fused : two_pass;
}

// ---------------------------------------------------------------------------
// The distance pass (:291 alone)
// ---------------------------------------------------------------------------
// Global-pointer schedule (the fp64/fp16/bf16 passes and the probe
// variants): 32 x 16-B loads in flight per thread (U4 x C8) in one launch;
// scripts/dist_variants.py (profiles/sweeps/r01_dist_*.jsonl) measured
// round-split launches within 1 % of it and U4 x C4 6 % behind.
constexpr int kDistCols = 8;
constexpr int kDistRows = 4;
// fp32 production (fedavg_client_sqdist_f32): the buffer-descriptor kernel at
// U2 x C16 in one launch -- full column groups read each row through one
// SGPR descriptor with no masking, 64 KiB contiguous per row per block, the
// reduce's winning shape: 6,818-6,840 GB/s vs 6,520-6,531 for the
// global-pointer U4 x C8 (scripts/dist_variants.py, profiles/r02/dist_variants.jsonl).
// U4 x C8 remains the fp64/fp16/bf16 passes' schedule.  Each row's fp64 sum
// runs as 4 interleaved chains (slice j into chain j % 4, added pairwise):
// 0.9-1.5 % faster than one chain of 64 dependent square-adds in three
// interleaved runs, 8 chains no better, 16 slower; a one-row-ahead pipeline
// (U = 0) loses 5 % -- two rows in flight per wave beat compute overlap
// (profiles/r02/sweeps/dist_chains.jsonl).
constexpr int kDistBufRows = 2;
constexpr int kDistBufCols = 16;
constexpr int kDistBufChains = 4;
// 4 chains, at most one per slice
constexpr int dist_chains(int cols) { return cols < kDistBufChains ? cols : kDistBufChains; }

// The forms the fp32 production pass may name, {U, C} (client_sqdist_buf_kernel
// <U, C, 1, dist_chains(C)>); the only place they are written.
constexpr PlanEntry kDistBufForms[] = {{kDistBufRows, kDistBufCols}, {kDistRows, kDistCols}, {4, 4}, {8, 2}};

// fp32 production column groups per thread: 16 while that still gives two
// workgroups per CU (the 25M-column target: 1,526), else 4 while it gives
// ~one per CU, else 2.  A small model's rows are short, and at 16 slices the
// launch had 37 workgroups for resnet56 (100 x 600K) and 74 for FEMNIST
// (10 x 1.2M).  rocprofv3 kernel time (profiles/r02/sweeps/dist_small_models.json):
// resnet56 275 -> 72 us (U8 x C2), FEMNIST 30.8 -> 12.7 us (U4 x C4),
// cfg4 500 x 1M 1,383 -> 391 us (U4 x C4), 100 x 3.125M 309 -> 197 us (U4 x C4).
//
// Between them, U4 x C8 when the 16-slice launch would end in a partly
// filled round of workgroups: a launch of g groups on r resident slots runs
// ceil(g / r) rounds, so 685 groups (cfg4, 500 x 11.2M) on 512 slots of the
// 16-slice kernel (2 per CU) fill 67 %, against 89 % for the 1,371 8-slice
// groups on its 768 slots (3 per CU).  scripts/dist_variants.py
// (profiles/r02/sweeps/dist_many_clients*.jsonl): 500 x 11.2M 4.10 -> 3.69 ms,
// 1000 x 12.5M 8.49 -> 8.03, 200 x 10M 1.52 -> 1.26; 100 x 25M keeps 16
// slices (1,526 groups, 99 %; 1.467 vs 1.600 ms at 8).
inline double round_fill(int64_t groups, int64_t slots) {
  if (slots <= 0) return 0.0;
  const int64_t rounds = (groups + slots - 1) / slots;
  return static_cast<double>(groups) / static_cast<double>(rounds * slots);
}

// the entry of `forms` with C = cols ({0, 0}: none, which no launch walk finds)
template <size_t N>
constexpr PlanEntry dist_form(const PlanEntry (&forms)[N], int cols) {
  for (const PlanEntry& e : forms)
    if (e.b == cols) return e;
  return {0, 0};
}

// The fp32 production form for rows of P columns on `cus` CUs; slots16 /
// slots8: workgroups the chip keeps resident of the 16- and 8-slice forms.
inline PlanEntry dist_plan(int64_t P, int64_t cus, int64_t slots16, int64_t slots8) {
  const int64_t nvec = (P + 3) / 4;
  const int64_t g16 = (nvec + kReduceBlock * 16 - 1) / (kReduceBlock * 16);
  const int64_t g8 = (nvec + kReduceBlock * 8 - 1) / (kReduceBlock * 8);
  if (g16 >= 2 * cus) return dist_form(kDistBufForms, round_fill(g8, slots8) > round_fill(g16, slots16) + 0.05 ? 8 : 16);
  if (g8 >= slots8) return dist_form(kDistBufForms, 8);
  if ((nvec + kReduceBlock * 4 - 1) / (kReduceBlock * 4) >= cus * 9 / 10) return dist_form(kDistBufForms, 4);
  return dist_form(kDistBufForms, 2);
}

// fp64/fp16/bf16 passes: U4 x C8 while that gives ~one workgroup per CU,
// else U8 x C2 (the fp32 pass's short-row measurements, dist_plan)
constexpr int kDistSmallRows = 8;
constexpr int kDistSmallCols = 2;
constexpr PlanEntry kDistVecForms[] = {{kDistRows, kDistCols}, {kDistSmallRows, kDistSmallCols}};
inline PlanEntry dist_vec_plan(int64_t nvec, int64_t cus) {
  return dist_form(kDistVecForms, (nvec + kReduceBlock * kDistCols - 1) / (kReduceBlock * kDistCols) >= cus * 9 / 10
                                      ? kDistCols
                                      : kDistSmallCols);
}

// partials per row of a launch over nvec 16-B slices at `cols` per thread: one per wave
inline int64_t dist_waves(int64_t nvec, int cols) {
  const int64_t blocks = (nvec + kReduceBlock * cols - 1) / (kReduceBlock * cols);
  return blocks * (kReduceBlock / 64);
}

// fedavg_client_sqdist_workspace (K, P >= 1): production (`plan`: dist_plan); any variant of >= 4 slices
inline int64_t dist_workspace(int64_t K, int64_t P, const PlanEntry& plan) {
  return K * dist_waves((P + 3) / 4, plan.b < 4 ? plan.b : 4);
}

// 16-B slices of a row of P elements of elem_size bytes (2, 4 or 8; else 0)
inline int64_t dist_vec_slices(int64_t P, int64_t elem_size) {
  if (P <= 0 || (elem_size != 2 && elem_size != 4 && elem_size != 8)) return 0;
  const int64_t lanes = 16 / elem_size;
  return (P + lanes - 1) / lanes;
}
// fedavg_client_sqdist_workspace_elems: the fp64 / fp16 / bf16 pass's launch
inline int64_t dist_vec_workspace(int64_t K, int64_t P, int64_t elem_size, int64_t cus) {
  const int64_t nvec = dist_vec_slices(P, elem_size);
  if (K <= 0 || nvec <= 0) return 0;
  return K * dist_waves(nvec, dist_vec_plan(nvec, cus).b);
}

}  // namespace fedavg_impl
