// fedavg_client.hip -- the client's per-iteration statistics of fp32 models,
// part of libfedavg_amd.so.
//
// Client.train (client.py:52-86) keeps, next to forward and backward, a
// flattened copy of the weights and of the gradients of the previous local
// iteration and forms from them, every iteration, the :71 guard (NaN count,
// norm(grads), norm(last_w)) and the :78 / :82 norms norm(w - last_w) and
// norm(grads - last_grads): two torch.cat copies, a bool temporary, three
// P-sized differences and six norms, with a host sync per tensor truth test.
// Here one kernel walks the model's tensors where they lie together with a
// flat fp32 snapshot of the previous step and, per element, forms
//     d = fl32(cur - snap)                      (the fp32 difference of :78)
//     sum cur^2, sum d^2                        (squares and sums in fp64)
//     count of isnan(cur)
//     snap = cur
// moving 12 B per element (read cur, read snap, write snap).  The pass is
// client_pass.hpp's; this file holds the fp32 unit's loads and arithmetic, the
// kernels' entry points and the C ABI.  fedavg_client_track keeps the running rho / beta of :78-84
// on the device from two such records.
#include "client_pass.hpp"

namespace {
using namespace fedavg_impl;

// The fp32 unit keeps its own loads and arithmetic on f32x4 values: written
// as a rule of client_pass.hpp's unit (CvHalf / CvF64 are), the pass with a
// snapshot takes 68 VGPRs instead of 62 and loses a wave per SIMD.  The store,
// the unit's prologue and epilogue and the host side are the shared ones.
typedef CliElem<4> CliF32;

// elements [col, col + 4) of a unit of n columns of the model's tensor: one
// 16-B nontemporal load when the tensor is 16-B aligned and the slice is
// whole, else element by element (columns past n read as 0)
template <bool VEC>
__device__ __forceinline__ f32x4 load_cur(const float* p, int col, int n) {
  if (VEC && col + 4 <= n) return __builtin_nontemporal_load(to_global(reinterpret_cast<const f32x4*>(p + col)));
  const auto q = to_global(p);
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  if (col < n) v.x = __builtin_nontemporal_load(q + col);
  if (col + 1 < n) v.y = __builtin_nontemporal_load(q + col + 1);
  if (col + 2 < n) v.z = __builtin_nontemporal_load(q + col + 2);
  if (col + 3 < n) v.w = __builtin_nontemporal_load(q + col + 3);
  return v;
}

// the snapshot's slice (16-B aligned: key offsets are multiples of 4)
__device__ __forceinline__ f32x4 load_snap(const float* p, int col, int n) {
  if (col + 4 <= n) return *reinterpret_cast<const f32x4*>(p + col);
  f32x4 v{0.f, 0.f, 0.f, 0.f};
  if (col < n) v.x = p[col];
  if (col + 1 < n) v.y = p[col + 1];
  if (col + 2 < n) v.z = p[col + 2];
  return v;
}

__device__ __forceinline__ double sq4_add(double acc, f32x4 d) {
  const double x = d.x, y = d.y, z = d.z, w = d.w;  // the fp64 square of an fp32 value is exact
  acc = __builtin_fma(x, x, acc);
  acc = __builtin_fma(y, y, acc);
  acc = __builtin_fma(z, z, acc);
  return __builtin_fma(w, w, acc);
}

__device__ __forceinline__ int nan4(f32x4 c) {
  return static_cast<int>(c.x != c.x) + static_cast<int>(c.y != c.y) + static_cast<int>(c.z != c.z) +
         static_cast<int>(c.w != c.w);
}

// one unit: this thread's kCliC slices; acc = {NaN count, sum cur^2, sum d^2}
template <bool HAS, bool VEC>
__device__ __forceinline__ void client_unit(const float* __restrict__ cur, float* __restrict__ snap, int n,
                                            double (&acc)[kClientStats]) {
  f32x4 cv[kCliC], sv[kCliC];
#pragma unroll
  for (int s = 0; s < kCliC; ++s) cv[s] = load_cur<VEC>(cur, cli_col<CliF32>(s), n);
  if constexpr (HAS) {
#pragma unroll
    for (int s = 0; s < kCliC; ++s) sv[s] = load_snap(snap, cli_col<CliF32>(s), n);
  }
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCliC; ++s) {
    nans += nan4(cv[s]);
    acc[1] = sq4_add(acc[1], cv[s]);
    if constexpr (HAS) acc[2] = sq4_add(acc[2], cv[s] - sv[s]);  // fp32 difference, as w - last_w at :78
    cli_store<CliF32, CliSnapshot, true>(snap, cli_col<CliF32>(s), n, __builtin_bit_cast(CliSlice, cv[s]));
  }
  acc[0] = static_cast<double>(nans);
}

template <bool HAS>
__global__ __launch_bounds__(kBlock) void client_stats_f32_kernel(const ClientKey* __restrict__ keys, int64_t n_keys,
                                                                  float* __restrict__ snap,
                                                                  double* __restrict__ partials, int64_t units) {
  const CliUnit<ClientKey> un = cli_unit<CliF32>(keys, n_keys);
  const float* cur = reinterpret_cast<const float*>(un.key.ptr) + un.c0;
  float* sn = snap + un.key.snap_offset + un.c0;
  double acc[kClientStats] = {0.0, 0.0, 0.0};
  if ((un.key.ptr & 15) == 0)
    client_unit<HAS, true>(cur, sn, un.n, acc);
  else
    client_unit<HAS, false>(cur, sn, un.n, acc);
  cli_store_partials(acc, partials, units);
}

__global__ __launch_bounds__(kBlock) void client_stats_finalize_kernel(const double* __restrict__ partials,
                                                                       int64_t units, double* __restrict__ stats) {
  cli_finalize(partials, units, stats);
}

// client.py:78-84 on the device (client_pass.hpp's cli_track in fp32).  The
// state holds fp32 values in doubles.
__global__ __launch_bounds__(64) void client_track_kernel(double* __restrict__ state, const double* __restrict__ w_stats,
                                                          const double* __restrict__ g_stats, double abs_dloss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  cli_track<CliOpF32>(state, w_stats, g_stats, abs_dloss);
}

int bad_tensor(const char* what, int64_t key, int64_t) {
  return set_error(FEDAVG_EINVAL, "%s: key %lld: null or misaligned tensor", what, (long long)key);
}

const ClientLib kLib = {set_error, launch_status, client_stats_finalize_kernel, bad_tensor};

}  // namespace

extern "C" {

int64_t fedavg_client_stats_workspace(int64_t n_keys) { return client_workspace(n_keys); }

int64_t fedavg_client_stats_partials(const int64_t* key_numel, int64_t n_keys) {
  return client_partials(key_numel, n_keys, client_span(4));
}

int fedavg_client_stats_f32(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, float* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream) {
  return client_stats_entry<CliF32>(kLib, "fedavg_client_stats_f32",
                                    {client_stats_f32_kernel<false>, client_stats_f32_kernel<true>}, cur_ptrs,
                                    key_numel, key_offset, n_keys, snap, P, has_snap, partials, partial_elems, stats,
                                    host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_track(double* state, const double* w_stats, const double* g_stats, double abs_dloss, void* stream) {
  return client_track_entry(kLib, "fedavg_client_track", client_track_kernel, state, w_stats, g_stats, abs_dloss,
                            stream);
}

}  // extern "C"
