// client_pass_plan.hpp -- the host arithmetic of the three client passes
// (fedavg_client.hip, fedavg_client_vec.hip, fedavg_client_step.hip through
// client_pass.hpp; HIP-free, also g++-built by tests/native/
// client_pass_check.cpp): the unit count, the two staged key tables, the bytes
// the one H2D ships and the checks of a key list.
//
// A key is one tensor of the model.  Each key is cut into units of 16 KiB of
// the tensor (4,096 fp32 / 8,192 16-bit / 2,048 fp64 elements), one workgroup
// each; unit_start is the key's first unit, nondecreasing along the table, so
// a workgroup finds its key as the last one with unit_start <= its index (an
// empty key shares its unit_start with the key after it and is never found).
#pragma once

#include <cstdint>

namespace fedavg_impl {

// the staged table entries, 32 B each: the statistics' (tensor address,
// elements, snapshot offset, first unit) and the step's (weight address,
// gradient address, elements, first unit)
struct ClientKey {
  int64_t ptr, numel, snap_offset, unit_start;
};
struct StepKey {
  int64_t w, g, numel, unit_start;
};
static_assert(sizeof(ClientKey) == 32 && sizeof(StepKey) == 32, "staged layout");

constexpr int64_t kClientUnitBytes = 256 * 4 * 16;  // 256 threads x 4 slices of 16 B
constexpr int kClientStats = 3;                     // partial sums per workgroup

// elements of one unit; 0 for an element size no pass has a kernel for (which
// of these sizes a library accepts is the library's own rule)
constexpr int64_t client_span(int64_t elem_size) {
  return elem_size == 4 || elem_size == 2 || elem_size == 8 ? kClientUnitBytes / elem_size : 0;
}

constexpr int64_t client_units_of(int64_t numel, int64_t span) { return numel > 0 ? (numel + span - 1) / span : 0; }

// bytes of the staged table: what host_ws and dev_ws hold and the H2D ships
constexpr int64_t client_workspace(int64_t n_keys) { return n_keys > 0 ? n_keys * 32 : 0; }

// units of a key list (keys without elements take none)
inline int64_t client_units(const int64_t* numel, int64_t n_keys, int64_t span) {
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) units += client_units_of(numel[j], span);
  return units;
}

// doubles of the partials buffer; 0 for no list, no key or no span
inline int64_t client_partials(const int64_t* numel, int64_t n_keys, int64_t span) {
  if (!numel || n_keys <= 0 || span == 0) return 0;
  return kClientStats * client_units(numel, n_keys, span);
}

// what one fill found: the units, and the first and last key with elements (-1: none)
struct ClientFill {
  int64_t units, first, last;
};

// hk[j] = entry(j, unit_start) for j in [0, n_keys): client_workspace(n_keys) bytes and not one more
template <class Key, class Entry>
inline ClientFill client_fill(Key* hk, const int64_t* numel, int64_t n_keys, int64_t span, Entry entry) {
  ClientFill f{0, -1, -1};
  for (int64_t j = 0; j < n_keys; ++j) {
    hk[j] = entry(j, f.units);
    f.units += client_units_of(numel[j], span);
    if (numel[j] > 0) {
      if (f.first < 0) f.first = j;
      f.last = j;
    }
  }
  return f;
}

// ---------------------------------------------------------------------------
// The checks of a key list: which one failed first and for which key (the
// library words the message).  es: element bytes (2, 4 or 8).
// ---------------------------------------------------------------------------
enum ClientBad {
  kClientOk = 0,
  kClientNegative,      // a key of negative size (the step)
  kClientOutside,       // a key that does not lie inside the snapshot of P elements (the statistics)
  kClientBadTensor,     // a key with elements whose address is null or no multiple of es
  kClientBadOffset,     // a snapshot offset that is no multiple of 16 / es elements
  kClientTooManyUnits,  // more units than a grid holds (key = -1)
};

struct ClientCheck {
  ClientBad bad;
  int64_t key;    // the first key that fails, -1 when it is the list as a whole
  int64_t units;  // of the whole list, when nothing failed
};

constexpr bool client_bad_tensor(int64_t numel, int64_t ptr, int64_t es) {
  return numel > 0 && (ptr == 0 || (ptr & (es - 1)) != 0);
}

constexpr ClientCheck client_checked_units(int64_t units) {
  return units > INT32_MAX ? ClientCheck{kClientTooManyUnits, -1, units} : ClientCheck{kClientOk, -1, units};
}

// the statistics' keys, in key order: inside the snapshot, then the tensor's address
inline ClientCheck client_check_stats_keys(const int64_t* ptrs, const int64_t* numel, const int64_t* offset,
                                           int64_t n_keys, int64_t P, int64_t es) {
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) {
    const int64_t n = numel[j], off = offset[j];
    if (n < 0 || off < 0 || off > P || n > P - off) return {kClientOutside, j, 0};
    if (client_bad_tensor(n, ptrs[j], es)) return {kClientBadTensor, j, 0};
    units += client_units_of(n, client_span(es));
  }
  return client_checked_units(units);
}

// the snapshot side is read 16 B at a time: every key starts on a 16-B boundary of it
inline ClientCheck client_check_snap_offsets(const int64_t* offset, int64_t n_keys, int64_t es) {
  for (int64_t j = 0; j < n_keys; ++j)
    if (offset[j] % (16 / es)) return {kClientBadOffset, j, 0};
  return {kClientOk, -1, 0};
}

// the step's keys, in key order: the size, then both addresses
inline ClientCheck client_check_step_keys(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* numel,
                                          int64_t n_keys, int64_t es) {
  for (int64_t j = 0; j < n_keys; ++j) {
    if (numel[j] < 0) return {kClientNegative, j, 0};
    if (client_bad_tensor(numel[j], w_ptrs[j], es) || client_bad_tensor(numel[j], g_ptrs[j], es))
      return {kClientBadTensor, j, 0};
  }
  return client_checked_units(client_units(numel, n_keys, client_span(es)));
}

}  // namespace fedavg_impl
