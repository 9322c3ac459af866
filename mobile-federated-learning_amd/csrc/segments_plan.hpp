// segments_plan.hpp -- host arithmetic of the zero-copy passes over device-resident clients
// (fedavg_segments.hip): unit widths and schedules, the unfused passes' plans and form tables, the
// fused pass's plan, the partials' bounds.  HIP-free on purpose, as reduce_plan.hpp: the CU count
// is an argument and the kernels' residency a callable, parts(plan, K, units) = the partials' second
// dimension of the plan's launch over `units` units (0: no instance, or not resident).
// fedavg_segments.hip passes its instance tags' occupancy queries, tests/native/segments_plan_check.cpp
// (g++, ASan + UBSan) a fixed table, against tests/segments_plan_cases.txt.
#pragma once

#include <algorithm>
#include <cstdint>

#include "plan_table.hpp"
#include "staging.hpp"

namespace fedavg_impl {

// the one plan struct of a zero-copy round: {win, kmax, span, small, waves}
using fedavg_staging::RoundPlan;

constexpr int kSegBlock = 256;  // threads per workgroup of the unit kernels (common.hpp's kBlock)

// U4 x C4: units of 4,096 columns.  The multi-key sweep (scripts/
// segments_probe.py --model, profiles/r01_segments_models.jsonl) measured
// resnet56 x 100 at 113 us against 161 us for U4 x C8 (more units for the
// mid-size keys, cheaper masked tails), FEMNIST 19.1 vs 20.2 us, and the flat
// 25M-element key level (6,256 vs 6,226 GB/s); U2 x C16 loses 2.7x on resnet56.
constexpr int kSegU = 4, kSegC = 4;
constexpr int64_t kSegSpan = static_cast<int64_t>(kSegBlock) * kSegC * 4;  // columns per unit
// Round 3: full units run reduce_raw_unit's STYLE 2 -- loads and products
// interleaved in (row, slice) order with two loads of the wave in flight
// (a sched_barrier keeps the compiler from bunching a batch's loads) -- in
// launches of 2 workgroups per CU.  Interleaved against the round-2 schedule
// (U4 x C4, batch loads, 3 per CU) on separately allocated client tensors
// (scripts/segments_probe.py --model, profiles/r03/seg/models.jsonl): flat
// 100 x 25M 1.580 -> 1.444 ms (6,393 -> 6,996 GB/s), resnet18_gn x 500
// (62 keys) 3.683 -> 3.285 ms, resnet56 x 100 (small units, 8 per CU)
// 101.8 -> 94.6 us, FEMNIST x 10 17.4 -> 17.2 us; 3 per CU 1.479 ms, 4 loads
// in flight 1.498 ms, 64 KiB units (U2 x C16, 1 per CU) 1.473 ms.
constexpr int kSegStyle = 2, kSegBlocksPerCU = 2;
// Small models (fewer than 4 units of 4,096 columns per CU): units of 1,024
// columns (U4 x C1), up to 8 blocks per CU per launch -- 4x the workgroups.
// rocprofv3 kernel time per call (scripts/segments_probe.py --model,
// profiles/r02/sweeps/segments_small_models.json): resnet56 x 100 (350 keys)
// 90.0 -> 77.1 us, FEMNIST x 10 12.1 -> 10.9 us, MNIST-LR x 10 6.3 -> 4.3 us;
// the flat 25M key stays on C4 (1,577 vs 1,717 us at C1).
constexpr int kSegSmallC = 1, kSegSmallBlocksPerCU = 8;
constexpr int64_t kSegSmallUnitsPerCU = 4;
constexpr int64_t kSegSmallSpan = static_cast<int64_t>(kSegBlock) * kSegSmallC * 4;
// :291 on device-resident clients: U4 client rows per load batch; units of
// 8,192 columns (C8), or the small-model units of 1,024 (C1).  rocprofv3
// kernel time (scripts/segments_dist_probe.py, profiles/r02/sweeps/
// segments_dist.json): flat 100 x 25M 1,638 us at U4 x C8 vs 1,656 for the
// round-1 form (one client at a time, C4) and 1,681 at U4 x C4; resnet56 x 100
// 84.5 us at U4 x C1 vs 100.8 (one client at a time, C4); FEMNIST 13.8 vs 14.5.
constexpr int kSegDistU = 4, kSegDistC = 8;
constexpr int64_t kSegDistSpan = static_cast<int64_t>(kSegBlock) * kSegDistC * 4;
constexpr int64_t kSegSpanMaxBytes = static_cast<int64_t>(kSegBlock) * 16 * 16;  // widest unit (C = 16), bytes

inline int64_t units_of(const int64_t* numel, int64_t n_keys, int64_t span = kSegSpan) {
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) units += (numel[j] + span - 1) / span;
  return units;
}

// a model with fewer than kSegSmallUnitsPerCU units of kSegSpan per CU takes
// the narrow units (reduce and :291 alike)
inline bool segments_small(const int64_t* numel, int64_t n_keys, int64_t cus) {
  if (!numel || n_keys <= 0) return false;
  for (int64_t j = 0; j < n_keys; ++j)
    if (numel[j] < 0) return false;  // stage_tables reports it
  return units_of(numel, n_keys) < kSegSmallUnitsPerCU * cus;
}

// The unfused passes (the reduce, the pointer reduce, the :291 pass): U client
// rows per batch x C 16-B slices per thread on units of `span` columns, in
// round-split launches of blocks_per_cu x CUs workgroups (0: one launch).
// The forms a plan may name, {U, C}: the only place they are written.
struct SegPassPlan {
  int unroll, cols, blocks_per_cu;
  int64_t span;
};
constexpr PlanEntry kSegReduceForms[] = {{kSegU, kSegSmallC}, {kSegU, kSegC}};
constexpr PlanEntry kSegDistForms[] = {{kSegDistU, kSegSmallC}, {kSegDistU, kSegDistC}};
#ifdef FEDAVG_TUNING  // probe library only: the (U, C) the two _variant entry points take
constexpr PlanEntry kSegReduceVariants[] = {{4, 8}, {8, 4}, {2, 8}, {4, 4}, {8, 2}, {16, 2}, {2, 16}, {1, 16}};
constexpr PlanEntry kSegDistVariants[] = {{1, 4}, {4, 4}, {8, 4}, {4, 1}, {8, 1}, {4, 2}, {8, 2}, {4, 8}};
#endif
constexpr int64_t seg_span_of(int cols) { return static_cast<int64_t>(kSegBlock) * cols * 4; }

inline SegPassPlan segments_reduce_plan(bool small) {
  return small ? SegPassPlan{kSegU, kSegSmallC, kSegSmallBlocksPerCU, kSegSmallSpan}
               : SegPassPlan{kSegU, kSegC, kSegBlocksPerCU, kSegSpan};
}
inline SegPassPlan segments_dist_plan(bool small) {
  return small ? SegPassPlan{kSegDistU, kSegSmallC, 0, kSegSmallSpan}
               : SegPassPlan{kSegDistU, kSegDistC, 0, kSegDistSpan};
}
inline RoundPlan segments_round_plan(const int64_t* numel, int64_t n_keys, int64_t cus) {
  const bool small = segments_small(numel, n_keys, cus);
  return RoundPlan{false, 0, segments_reduce_plan(small).span, small};
}

// fedavg_segments_partials: one partial per wave of every unit of the :291 pass
inline int64_t segments_dist_partials(const int64_t* numel, int64_t n_keys, int64_t K, int64_t cus) {
  if (!numel || n_keys <= 0 || K <= 0) return 0;
  return K * units_of(numel, n_keys, segments_dist_plan(segments_small(numel, n_keys, cus)).span) * (kSegBlock / 64);
}

// The fused pass (aggregate + :291 in one read): LDS-DMA tiles (kSegTiles),
// one-wave windows (kWinBands) or split-row windows (kSplitForms).
// Round 3 ran 81-100 clients on the 128 x 1 window instance because its
// 100 x 2 form spilled (device round 100 x 25M 3.66 ms, profiles/r03/segwin/);
// the spill was the slow path's per-lane 64-bit element addresses, gone with
// the buffer-load form (232 VGPRs, no scratch), so 81-100 clients take 100 x 2
// as on rows (kWinBands, plan_table.hpp)
constexpr int kSegFusedMaxK = kSegBlock;  // the tile kernel loads at most one client address per thread
constexpr int64_t kSegSplitMaxK = 1024;   // the split-row windows' reach (16 waves of 64 clients)
constexpr int64_t kSegWinMinPerWave = 16;  // windows per wave below which the LDS-DMA tiles keep the round
// 129-256 clients take the zero-copy split windows too when every workgroup
// gets >= kSegSplitMinPerBlock windows (round 6; profiles/r06/seg160/, seg129/,
// resnet18_gn-shaped device rounds, ms, tiles vs split windows: 129 2.07 vs
// 1.46; 150 2.29 vs 1.49; 160 2.44 vs 1.43; 200 2.90 vs 1.71; 256 4.12 vs
// 2.10; the one-wave windows keep <= 128: 100 0.79 vs 1.06, 120 0.97 vs 1.11)
constexpr int64_t kSegSplitMinK = 129, kSegSplitMinPerBlock = 8;

// what the probe library may override (the product library default-constructs
// it): windows off = the LDS-DMA tiles for every round, and the two thresholds
struct SegKnobs {
  bool windows = true;
  int64_t win_min_per_wave = kSegWinMinPerWave, split_min_k = kSegSplitMinK;
};

// tile width by clients (32 above 128, 64 above 64, 128 up to 64, 256 up to
// 16): every width keeps <= 8 load slots per thread; kSegTiles: the widths, f(S)
inline int seg_fused_cols(int64_t K) { return K > 128 ? 32 : (K > 64 ? 64 : (K > 16 ? 128 : 256)); }
constexpr PlanEntry kSegTiles[] = {{32, 0}, {64, 0}, {128, 0}, {256, 0}};
inline int64_t seg_fused_lds_bytes(int64_t K, int S, bool laddr = false) {
  const int64_t b = (K + 1) * S * 4 + (laddr ? K * 8 : 0);  // LADDR: + the key's K client addresses
  return b > kSegBlock * 8 ? b : kSegBlock * 8;
}

// 257-1024 clients fuse only on the split-row windows: 32-bit buffer offsets
// per key, window indices in 32 bits
inline bool seg_split_ok(const int64_t* numel, int64_t n_keys) {
  if (!numel || n_keys <= 0 || n_keys >= (int64_t(1) << 31)) return false;
  for (int64_t j = 0; j < n_keys; ++j)
    if (numel[j] < 0 || numel[j] >= (int64_t(1) << 30)) return false;
  return units_of(numel, n_keys, 64) < (int64_t(1) << 31);
}

inline RoundPlan seg_split_plan() { return RoundPlan{true, -1, 64, false}; }  // kmax -1: the split-row windows
inline RoundPlan seg_tile_plan(int64_t K) { return RoundPlan{false, 0, seg_fused_cols(K), false}; }
inline RoundPlan seg_win_plan(const PlanEntry& band) { return RoundPlan{true, band.a, 64 * band.b, false}; }

// The fused pass a round takes: the wave-owned windows for 17-128 clients
// when every key is fp32 and each wave gets at least win_min_per_wave
// windows, the split-row windows from split_min_k clients when every
// workgroup gets kSegSplitMinPerBlock windows (beyond kSegFusedMaxK: always),
// else the LDS-DMA tiles.
template <class Parts>
RoundPlan seg_fused_plan(const int64_t* numel, int64_t n_keys, int64_t K, bool all_raw, const SegKnobs& knobs,
                         Parts&& parts) {
  const PlanEntry* band = win_band_of(K);  // {KMAX, VEC}, nullptr outside 17..128
  RoundPlan p = seg_tile_plan(K);
  p.kmax = band ? band->a : 0;
  const RoundPlan split = seg_split_plan();
  if (K >= knobs.split_min_k && K >= 2 && K <= kSegFusedMaxK && all_raw && seg_split_ok(numel, n_keys)) {
    const int64_t units = units_of(numel, n_keys, 64);
    const int64_t blocks = parts(split, K, units);
    if (blocks > 0 && units >= kSegSplitMinPerBlock * blocks) {
      p = split;
      p.waves = blocks;
      return p;
    }
  }
  if (K > kSegFusedMaxK) {
    if (K <= kSegSplitMaxK && all_raw && seg_split_ok(numel, n_keys)) {
      p = split;
      p.waves = parts(split, K, units_of(numel, n_keys, 64));
    }
    return p;
  }
  // the windows address a key's bytes with 32-bit buffer offsets
  bool small_keys = numel != nullptr;
  for (int64_t j = 0; small_keys && j < n_keys; ++j) small_keys = numel[j] < (int64_t(1) << 30);
  if (band && all_raw && small_keys && n_keys > 0 && n_keys < (int64_t(1) << 31) && knobs.windows) {
    const RoundPlan win = seg_win_plan(*band);
    const int64_t wunits = units_of(numel, n_keys, win.span);
    const int64_t waves = parts(win, K, wunits);
    if (waves > 0 && wunits >= knobs.win_min_per_wave * waves && wunits < (int64_t(1) << 31)) {
      p = win;
      p.waves = waves;
    }
  }
  return p;
}

// fedavg_reduce_sqdist_segments_partials: K x the widest launch any plan of K
// clients can take (`extra`: the probe library's timeline stamps)
template <class Parts>
int64_t seg_fused_partials(int64_t K, const SegKnobs& knobs, int64_t extra, Parts&& parts) {
  if (K <= 0 || K > kSegSplitMaxK) return 0;
  const int64_t full = INT64_MAX / 2;  // units of a launch that fills the chip
  const int64_t split = parts(seg_split_plan(), K, full);
  if (K > kSegFusedMaxK) return K * split + extra;  // the split-row windows (device round)
  const PlanEntry* band = win_band_of(K);
  const int64_t tiles = parts(seg_tile_plan(K), K, full);
  const int64_t windows = band ? parts(seg_win_plan(*band), K, full) : 0;
  const int64_t need = std::max(std::max(tiles, windows), K >= knobs.split_min_k ? split : 0);  // 129-256: split too
  return K * need + extra;
}

}  // namespace fedavg_impl
