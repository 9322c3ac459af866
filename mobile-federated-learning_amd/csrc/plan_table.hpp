// plan_table.hpp -- plan tables (host, HIP-free).  A plan family is one
// constexpr table of {a, b} template arguments; for_entry calls a generic
// lambda with the matching entry's two values as std::integral_constants and
// says whether there was one, so the lambda is instantiated for the table's
// entries and nothing else (the product library holds plan-reachable kernels
// only), and every use of a family -- plan, grid, workspace, launch -- names
// its instances through the same table.  Tables: here (the window kernels'
// bands and grid rules, for window.hpp and segments_plan.hpp alike),
// reduce_plan.hpp (the row reduce's forms), segments_plan.hpp (the zero-copy
// passes'), dist_plan.hpp (the rows passes') and the translation units' own.
#pragma once

#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>

namespace fedavg_impl {

struct PlanEntry {
  int a, b;
};
constexpr int kAnyB = -1;

template <auto& T, class F, size_t... I>
bool for_entry_impl(int a, int b, F&& f, std::index_sequence<I...>) {
  return ((a == T[I].a && (b == kAnyB || b == T[I].b) &&
           (f(std::integral_constant<int, T[I].a>{}, std::integral_constant<int, T[I].b>{}), true)) ||
          ...);
}
template <auto& T, class F>
bool for_entry(int a, int b, F&& f) {
  return for_entry_impl<T>(a, b, f, std::make_index_sequence<std::extent_v<std::remove_reference_t<decltype(T)>>>{});
}

// Plan tables of the window kernels (fedavg_dist.hip's [K, ld] rows and
// fedavg_segments.hip's zero-copy forms).
// One-wave windows, 17..128 rows: {KMAX, VEC} by band (measurements:
// dist_plan.hpp's fused_plan notes).  The only place the bands are written.
constexpr PlanEntry kWinBands[] = {{48, 4}, {64, 2}, {80, 2}, {100, 2}, {128, 1}};
constexpr int64_t kWinMinK = 17;

// the band of K rows ({kmax, vec}), nullptr outside 17..128
inline const PlanEntry* win_band_of(int64_t K) {
  if (K < kWinMinK) return nullptr;
  for (const PlanEntry& b : kWinBands)
    if (K <= b.a) return &b;
  return nullptr;
}
// f(KMAX, VEC) for the band whose KMAX is `kmax`; false: no such band
template <class F>
bool for_win_band(int kmax, F&& f) {
  return for_entry<kWinBands>(kmax, kAnyB, f);
}

// Split-row windows (hand-off form): {NSMAX, PF} -- up to 8 waves per
// workgroup with 8 prefetched rows, up to 16 with 16 (profiles/r06/winf/)
constexpr PlanEntry kSplitForms[] = {{8, 8}, {16, 16}};
// f(NSMAX, PF) for workgroups of (at most) `waves` waves
template <class F>
bool for_split(int waves, F&& f) {
  return for_entry<kSplitForms>(waves <= 8 ? 8 : 16, kAnyB, f);
}

// The grid rules of every fused aggregate + :291 launcher.  The CU count is
// an argument: fedavg_fused_vec.hip sizes its grids for a constant chip and
// answers without a device, and the sanitizer checks have none.
// Workgroups per CU of a split-row window launch: the resident ones rounded
// down to a power of two (3 workgroups of 5 waves on a CU ran 12-15 % slower
// than 2, profiles/r05/prefetch/; zero-copy: profiles/r06/zc_percu/); 0: none
inline int64_t split_per_cu(int64_t resident, int64_t cus) {
  const int64_t r = resident / cus;
  int64_t per_cu = 0;
  if (r >= 1)
    for (per_cu = 1; per_cu * 2 <= r;) per_cu *= 2;
  return per_cu;
}
// workgroups of a persistent launch: every resident one, or one per work item
// when there are fewer
inline int64_t persistent_grid(int64_t per_cu, int64_t cus, int64_t items) {
  const int64_t g = per_cu * cus;
  return items < g ? items : g;
}
// waves of a window launch of NW-wave workgroups: a workgroup per NW windows
inline int64_t window_waves(int64_t per_cu, int64_t cus, int64_t windows, int nw) {
  return persistent_grid(per_cu, cus, (windows + nw - 1) / nw) * nw;
}

}  // namespace fedavg_impl
