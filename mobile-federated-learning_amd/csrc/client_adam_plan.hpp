// client_adam_plan.hpp -- the host arithmetic of the client's Adam step
// (fedavg_client_adam.hip) that client_pass_plan.hpp does not already hold:
// the staged key entry of five fields, the bytes of its table, and the checks
// of a key list against the optimizer state.  HIP-free, like that header.
//
// The state is one buffer of the model's type: three planes (exp_avg,
// exp_avg_sq, max_exp_avg_sq) of state_elems elements each.  Key j sits
// state_offset[j] elements into every plane, a multiple of 16 B, so the state
// is read and written 16 B at a time whatever the tensors' own alignment.
#pragma once

#include "client_pass_plan.hpp"

namespace fedavg_impl {

// the staged table entry, 40 B: (weight address, gradient address, elements,
// offset in a state plane, first unit)
struct AdamKey {
  int64_t w, g, numel, state_offset, unit_start;
};
static_assert(sizeof(AdamKey) == 40, "staged layout");

constexpr int kAdamCoefs = 7;      // wd, 1 - beta1, beta2, 1 - beta2, sqrt(1 - beta2^t), eps, -lr / (1 - beta1^t)
constexpr int kAdamSites = 4;      // the x + s * y sites a form mask has a bit for
constexpr int kAdamStatePlanes = 3;

// bytes of the staged table: what host_ws and dev_ws hold and the H2D ships
constexpr int64_t adam_workspace(int64_t n_keys) {
  return n_keys > 0 ? n_keys * static_cast<int64_t>(sizeof(AdamKey)) : 0;
}

constexpr bool adam_form_ok(int form) { return form >= 0 && form < (1 << kAdamSites); }

// Lerp.h takes `self + weight * (end - self)` only for |weight| < 0.5: the one branch the kernel has
// (a NaN weight is refused with the large ones)
inline bool adam_lerp_weight_ok(double lw) { return lw > -0.5 && lw < 0.5; }

// the step's keys, in key order: the size, both addresses, then the key's place in a state plane
// (kClientOutside: not inside [0, state_elems); kClientBadOffset: no multiple of 16 / es elements)
inline ClientCheck adam_check_keys(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* numel,
                                   const int64_t* offset, int64_t n_keys, int64_t state_elems, int64_t es) {
  for (int64_t j = 0; j < n_keys; ++j) {
    const int64_t n = numel[j], off = offset[j];
    if (n < 0) return {kClientNegative, j, 0};
    if (client_bad_tensor(n, w_ptrs[j], es) || client_bad_tensor(n, g_ptrs[j], es)) return {kClientBadTensor, j, 0};
    if (off < 0 || off > state_elems || n > state_elems - off) return {kClientOutside, j, 0};
    if (off % (16 / es)) return {kClientBadOffset, j, 0};
  }
  return client_checked_units(client_units(numel, n_keys, client_span(es)));
}

}  // namespace fedavg_impl
