// fedavg_client.hip -- the client's per-iteration statistics in one pass.
//
// Client.train (client.py:52-86) keeps, next to forward and backward, a
// flattened copy of the weights and of the gradients of the previous local
// iteration and forms from them, every iteration, the :71 guard (NaN count,
// norm(grads), norm(last_w)) and the :78 / :82 norms norm(w - last_w) and
// norm(grads - last_grads): two torch.cat copies, a bool temporary, three
// P-sized differences and six norms, with a host sync per tensor truth test.
// Here one kernel walks the model's tensors where they lie (a pointer table,
// as the zero-copy server kernels of fedavg_segments.hip do) together with a
// flat fp32 snapshot of the previous step and, per element, forms
//     d = fl32(cur - snap)                      (the fp32 difference of :78)
//     sum cur^2, sum d^2                        (squares and sums in fp64)
//     count of isnan(cur)
//     snap = cur
// moving 12 B per element (read cur, read snap, write snap).  Each key is cut
// into units of kCliSpan = 4,096 columns; a workgroup of 256 threads owns one
// unit, a thread 4 slices of 16 B (slice s at column 4 * (tid + 256 s)), with
// its 4 + 4 loads issued before the first use.  Snapshot key offsets are
// multiples of 4 elements, so the snapshot side is always 16-B accesses; a
// key whose tensor is 16-B aligned reads it with 16-B nontemporal loads, any
// other (4-B aligned) tensor element by element into the same slices, so both
// forms add the same values in the same order.  Every workgroup writes its
// three fp64 partials (wave sums by DPP, the 4 waves added in wave order); a
// one-workgroup finalize adds them in a fixed order: deterministic, no
// floating-point atomics.  fedavg_client_track keeps the running rho / beta
// of :78-84 on the device from two such records.
#include "common.hpp"

namespace {
using namespace fedavg_impl;

// the staged key table entry: tensor address, elements, snapshot offset, first unit
struct ClientKey {
  int64_t ptr, numel, snap_offset, unit_start;
};
static_assert(sizeof(ClientKey) == 32, "staged layout");

constexpr int kCliC = 4;                                                // 16-B slices per thread
constexpr int64_t kCliSpan = static_cast<int64_t>(kBlock) * kCliC * 4;  // columns per unit (4,096)
constexpr int kCliStats = 3;                                            // partial sums per workgroup

template <typename T>
using gptr = __attribute__((address_space(1))) const T*;

template <typename T>
__device__ __forceinline__ gptr<T> to_global(const void* p) {
  return (gptr<T>)(reinterpret_cast<uintptr_t>(p));
}

// elements [col, col + 4) of a unit of n columns of the model's tensor: one
// 16-B nontemporal load when the tensor is 16-B aligned and the slice is
// whole, else element by element (columns past n read as 0)
template <bool VEC>
__device__ __forceinline__ f32x4 load_cur(const float* p, int col, int n) {
  if (VEC && col + 4 <= n) return __builtin_nontemporal_load(to_global<f32x4>(p + col));
  const gptr<float> q = to_global<float>(p);
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

__device__ __forceinline__ void store_snap(float* p, int col, int n, f32x4 a) {
  if (col + 4 <= n) {
    *reinterpret_cast<f32x4*>(p + col) = a;
  } else if (col < n) {
    p[col] = a.x;
    if (col + 1 < n) p[col + 1] = a.y;
    if (col + 2 < n) p[col + 2] = a.z;
  }
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
                                            double (&acc)[kCliStats]) {
  f32x4 cv[kCliC], sv[kCliC];
#pragma unroll
  for (int s = 0; s < kCliC; ++s) cv[s] = load_cur<VEC>(cur, 4 * (static_cast<int>(threadIdx.x) + s * kBlock), n);
  if constexpr (HAS) {
#pragma unroll
    for (int s = 0; s < kCliC; ++s) sv[s] = load_snap(snap, 4 * (static_cast<int>(threadIdx.x) + s * kBlock), n);
  }
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCliC; ++s) {
    nans += nan4(cv[s]);
    acc[1] = sq4_add(acc[1], cv[s]);
    if constexpr (HAS) acc[2] = sq4_add(acc[2], cv[s] - sv[s]);  // fp32 difference, as w - last_w at :78
    store_snap(snap, 4 * (static_cast<int>(threadIdx.x) + s * kBlock), n, cv[s]);
  }
  acc[0] = static_cast<double>(nans);
}

// partials[i][u]: workgroup u's NaN count (i = 0), sum cur^2 (1), sum d^2 (2)
template <bool HAS>
__global__ __launch_bounds__(kBlock) void client_stats_f32_kernel(const ClientKey* __restrict__ keys, int64_t n_keys,
                                                                  float* __restrict__ snap,
                                                                  double* __restrict__ partials, int64_t units) {
  __shared__ double red[kCliStats][kBlock / 64];
  const int64_t u = blockIdx.x;
  const int64_t j = wave_search_last_le([&](int64_t x) { return keys[x].unit_start; }, n_keys, u);
  const ClientKey key = keys[j];
  const int64_t c0 = (u - key.unit_start) * kCliSpan;
  const int n = static_cast<int>(key.numel - c0 < kCliSpan ? key.numel - c0 : kCliSpan);
  const float* cur = reinterpret_cast<const float*>(key.ptr) + c0;
  float* sn = snap + key.snap_offset + c0;
  double acc[kCliStats] = {0.0, 0.0, 0.0};
  if ((key.ptr & 15) == 0)
    client_unit<HAS, true>(cur, sn, n, acc);
  else
    client_unit<HAS, false>(cur, sn, n, acc);
#pragma unroll
  for (int i = 0; i < kCliStats; ++i) {
    const double w = wave_sum_dpp(acc[i]);
    if ((threadIdx.x & 63u) == 0) red[i][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < kCliStats) {
    double s = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
    partials[static_cast<int64_t>(threadIdx.x) * units + u] = s;
  }
}

// stats[i] = sum over the workgroups' partials in a fixed order; stats[3] = 0
__global__ __launch_bounds__(kBlock) void client_stats_finalize_kernel(const double* __restrict__ partials,
                                                                       int64_t units, double* __restrict__ stats) {
  __shared__ double red[kBlock];
  for (int i = 0; i < kCliStats; ++i) {
    double s = 0.0;
    for (int64_t w = threadIdx.x; w < units; w += kBlock) s += partials[i * units + w];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
      if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) stats[i] = red[0];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[3] = 0.0;
}

// client.py:78-84 on the device.  Every fp32 operation is formed in fp64 from
// fp32 operands and rounded once to fp32: for sqrt, a quotient and a product
// of fp32 values that is the correctly rounded fp32 result (53 >= 2 * 24 + 2).
__device__ __forceinline__ void track_update(double* __restrict__ x, double* __restrict__ has, float tmp) {
  const float cur = static_cast<float>(*x);
  if (*has == 0.0 || cur == 0.0f || tmp > cur) *x = static_cast<double>(tmp);  // `not x or tmp > x` (:79, :83)
  *has = 1.0;
}

__global__ __launch_bounds__(64) void client_track_kernel(double* __restrict__ state, const double* __restrict__ w_stats,
                                                          const double* __restrict__ g_stats, double abs_dloss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float n_w = static_cast<float>(__builtin_sqrt(w_stats[2]));  // norm(w - last_w)
  const float n_g = static_cast<float>(__builtin_sqrt(g_stats[2]));  // norm(grads - last_grads)
  const float recip = static_cast<float>(1.0 / static_cast<double>(n_w));
  const float dl = static_cast<float>(abs_dloss);
  const float rho_tmp = static_cast<float>(static_cast<double>(recip) * static_cast<double>(dl));
  const float beta_tmp = static_cast<float>(static_cast<double>(n_g) / static_cast<double>(n_w));
  track_update(state + 0, state + 2, rho_tmp);
  track_update(state + 1, state + 3, beta_tmp);
}

int64_t client_units(const int64_t* numel, int64_t n_keys) {
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j)
    if (numel[j] > 0) units += (numel[j] + kCliSpan - 1) / kCliSpan;
  return units;
}

int zero_stats(const char* what, double* stats, hipStream_t s) {
  if (!is_device_memory(stats)) return set_error(FEDAVG_EINVAL, "%s: stats must be device memory", what);
  const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(double), s);
  if (e == hipSuccess) return FEDAVG_OK;
  (void)hipGetLastError();
  return set_error(-static_cast<int>(e), "%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
}

}  // namespace

extern "C" {

int64_t fedavg_client_stats_workspace(int64_t n_keys) {
  return n_keys > 0 ? n_keys * static_cast<int64_t>(sizeof(ClientKey)) : 0;
}

int64_t fedavg_client_stats_partials(const int64_t* key_numel, int64_t n_keys) {
  if (!key_numel || n_keys <= 0) return 0;
  return kCliStats * client_units(key_numel, n_keys);
}

int fedavg_client_stats_f32(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, float* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream) {
  const char* what = "fedavg_client_stats_f32";
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0 || P < 0) return set_error(FEDAVG_EINVAL, "%s: negative n_keys or P", what);
  if (!stats) return set_error(FEDAVG_EINVAL, "%s: null stats", what);
  if (P == 0 || n_keys == 0) return zero_stats(what, stats, s);
  if (!cur_ptrs || !key_numel || !key_offset || !snap || !partials || !host_ws || !dev_ws)
    return set_error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = fedavg_client_stats_workspace(n_keys);
  if (ws_bytes < need_ws) return set_error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) {
    const int64_t n = key_numel[j], off = key_offset[j];
    if (n < 0 || off < 0 || off > P || n > P - off)
      return set_error(FEDAVG_EINVAL, "%s: key %lld lies outside the snapshot of %lld elements", what, (long long)j,
                       (long long)P);
    if (n > 0 && (cur_ptrs[j] == 0 || (cur_ptrs[j] & 3) != 0))
      return set_error(FEDAVG_EINVAL, "%s: key %lld: null or misaligned tensor", what, (long long)j);
    units += (n + kCliSpan - 1) / kCliSpan;
  }
  if (units > INT32_MAX) return set_error(FEDAVG_EINVAL, "%s: too many units", what);
  const int64_t need_parts = kCliStats * units;
  if (partial_elems < need_parts)
    return set_error(FEDAVG_EINVAL, "%s: partials need %lld doubles", what, (long long)need_parts);
  if (!aligned16(snap)) return set_error(FEDAVG_EALIGN, "%s: snap must be 16-B aligned", what);
  for (int64_t j = 0; j < n_keys; ++j)
    if (key_offset[j] & 3)
      return set_error(FEDAVG_EALIGN, "%s: key %lld: snapshot offset must be a multiple of 4 elements", what,
                       (long long)j);
  if (!aligned16(host_ws) || !aligned16(dev_ws) || (reinterpret_cast<uintptr_t>(partials) & 7u) ||
      (reinterpret_cast<uintptr_t>(stats) & 7u))
    return set_error(FEDAVG_EALIGN, "%s: workspaces must be 16-B, partials and stats 8-B aligned", what);
  if (units == 0) return zero_stats(what, stats, s);
  if (!is_pinned_host_memory(host_ws)) return set_error(FEDAVG_EINVAL, "%s: host_ws is not pinned host memory", what);
  if (!is_device_memory(dev_ws) || !is_device_memory(snap) || !is_device_memory(partials) || !is_device_memory(stats))
    return set_error(FEDAVG_EINVAL, "%s: dev_ws, snap, partials and stats must be device memory", what);
  // a host address would fault the kernel: spot check of the first and last
  // tensor (the Python layer checks every tensor's device)
  auto* hk = static_cast<ClientKey*>(host_ws);
  int64_t u0 = 0, first = -1, last = -1;
  for (int64_t j = 0; j < n_keys; ++j) {
    hk[j] = ClientKey{cur_ptrs[j], key_numel[j], key_offset[j], u0};
    u0 += (key_numel[j] + kCliSpan - 1) / kCliSpan;
    if (key_numel[j] > 0) {
      if (first < 0) first = j;
      last = j;
    }
  }
  if (!is_device_memory(reinterpret_cast<const void*>(cur_ptrs[first])) ||
      !is_device_memory(reinterpret_cast<const void*>(cur_ptrs[last])))
    return set_error(FEDAVG_EINVAL, "%s: the tensors must be device memory", what);
  const hipError_t e = hipMemcpyAsync(dev_ws, host_ws, static_cast<size_t>(need_ws), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_error(-static_cast<int>(e), "%s: hipMemcpyAsync failed: %s", what, hipGetErrorString(e));
  }
  const auto* keys = static_cast<const ClientKey*>(dev_ws);
  if (has_snap)
    hipLaunchKernelGGL(client_stats_f32_kernel<true>, dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, snap, partials, units);
  else
    hipLaunchKernelGGL(client_stats_f32_kernel<false>, dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, snap, partials, units);
  const int rc = launch_status(what);
  if (rc) return rc;
  hipLaunchKernelGGL(client_stats_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  return launch_status(what);
}

int fedavg_client_track(double* state, const double* w_stats, const double* g_stats, double abs_dloss, void* stream) {
  const char* what = "fedavg_client_track";
  if (!state || !w_stats || !g_stats) return set_error(FEDAVG_EINVAL, "%s: null argument", what);
  if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(w_stats) |
       reinterpret_cast<uintptr_t>(g_stats)) & 7u)
    return set_error(FEDAVG_EALIGN, "%s: records must be 8-B aligned", what);
  if (!is_device_memory(state) || !is_device_memory(w_stats) || !is_device_memory(g_stats))
    return set_error(FEDAVG_EINVAL, "%s: state and records must be device memory", what);
  hipLaunchKernelGGL(client_track_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, w_stats,
                     g_stats, abs_dloss);
  return launch_status(what);
}

}  // extern "C"
