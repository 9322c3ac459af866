// client_step_plan.hpp -- the host arithmetic of the fused client SGD step
// (fedavg_client_step.hip; HIP-free, also g++-built by
// tests/native/client_step_check.cpp): the unit count, the staged key table
// and the bytes the one H2D ships.
//
// A key is one tensor of the model: its weight and its gradient address and
// its elements.  Each key is cut into units of 16 KiB of the tensor (4,096
// fp32 / 8,192 16-bit / 2,048 fp64 elements), one workgroup each; unit_start
// is the key's first unit, nondecreasing along the table, so a workgroup finds
// its key as the last one with unit_start <= its index (an empty key shares
// its unit_start with the key after it and is never found).
#pragma once

#include <cstdint>

namespace fedavg_impl {

// the staged key table entry: weight address, gradient address, elements, first unit
struct StepKey {
  int64_t w, g, numel, unit_start;
};
static_assert(sizeof(StepKey) == 32, "staged layout");

constexpr int64_t kStepUnitBytes = 256 * 4 * 16;  // 256 threads x 4 slices of 16 B
constexpr int kStepStats = 3;                     // partial sums per workgroup

// elements of one unit; 0 for an element size the step has no kernel for
constexpr int64_t step_span(int64_t elem_size) {
  return elem_size == 4 || elem_size == 2 || elem_size == 8 ? kStepUnitBytes / elem_size : 0;
}

constexpr int64_t step_units_of(int64_t numel, int64_t span) { return numel > 0 ? (numel + span - 1) / span : 0; }

// bytes of the staged table: what host_ws and dev_ws hold and the H2D ships
constexpr int64_t step_workspace(int64_t n_keys) {
  return n_keys > 0 ? n_keys * static_cast<int64_t>(sizeof(StepKey)) : 0;
}

// units of a key list (keys without elements take none)
inline int64_t step_units(const int64_t* numel, int64_t n_keys, int64_t span) {
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) units += step_units_of(numel[j], span);
  return units;
}

// what one fill found: the units, and the first and last key with elements (-1: none)
struct StepFill {
  int64_t units, first, last;
};

// hk[0, n_keys): step_workspace(n_keys) bytes and not one more
inline StepFill step_fill(StepKey* hk, const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* numel,
                          int64_t n_keys, int64_t span) {
  StepFill f{0, -1, -1};
  for (int64_t j = 0; j < n_keys; ++j) {
    hk[j] = StepKey{w_ptrs[j], g_ptrs[j], numel[j], f.units};
    f.units += step_units_of(numel[j], span);
    if (numel[j] > 0) {
      if (f.first < 0) f.first = j;
      f.last = j;
    }
  }
  return f;
}

}  // namespace fedavg_impl
