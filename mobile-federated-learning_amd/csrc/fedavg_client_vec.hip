// fedavg_client_vec.hip -- libfedavg_amd_clientvec.so (include/
// fedavg_amd_clientvec.h): the client's per-iteration statistics in one pass
// for bf16, fp16 and fp64 models.
//
// fedavg_client.hip's pass (a staged key table, one workgroup of 256 threads
// per unit, wave search for the unit's key, DPP wave sums, three fp64 partials
// per workgroup, a one-workgroup finalize) with the unit templated on a dtype
// rule.  Per element of type T the pass forms
//     d = rT(f32(cur) - f32(snap))   bf16 / fp16: the difference in T (:78)
//     d = cur - snap                 fp64
//     sum cur^2, sum d^2             (squares and sums in fp64)
//     count of isnan(cur)
//     snap = cur                     (the bits, NaN payloads included)
// moving 6 B per 16-bit element and 24 B per fp64 element (read cur, read
// snap, write snap).  A unit is 16 KiB of a tensor: a thread owns 4 slices of
// 16 B (slice s at byte 16 * (tid + 256 s)), 8,192 elements of a 16-bit type
// or 2,048 of fp64, its 4 + 4 loads issued before the first use.  Snapshot key
// offsets are multiples of 16 B, so the snapshot side is always 16-B accesses;
// a key whose tensor is 16-B aligned reads it with 16-B nontemporal loads, any
// other tensor element by element into the same slices, so both forms add the
// same values in the same order.  Columns past the key's end read as zero and
// are never stored.  fedavg_client_track_{bf16,f16,f64} keep the running
// rho / beta of :78-84 on the device in the model's type.
#include "common.hpp"

#include "fedavg_amd_clientvec.h"

namespace {
using namespace fedavg_impl;

thread_local ErrorState g_cv_err;

int cv_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cv_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int cv_launch_status(const char* what) { return launch_status(g_cv_err, what); }

// the staged key table entry: tensor address, elements, snapshot offset, first unit
struct ClientKey {
  int64_t ptr, numel, snap_offset, unit_start;
};
static_assert(sizeof(ClientKey) == 32, "staged layout");

constexpr int kCvC = 4;                                            // 16-B slices per thread
constexpr int64_t kCvUnitBytes = static_cast<int64_t>(kBlock) * kCvC * 16;  // 16 KiB of the tensor per unit
constexpr int kCvStats = 3;                                        // partial sums per workgroup

template <typename T>
using gptr = __attribute__((address_space(1))) const T*;

template <typename T>
__device__ __forceinline__ gptr<T> to_global(const void* p) {
  return (gptr<T>)(reinterpret_cast<uintptr_t>(p));
}

// 16 B of a tensor as they lie in memory
struct CvSlice {
  unsigned int w[4];
};

__device__ __forceinline__ CvSlice cv_slice(u32x4 v) { return CvSlice{{v.x, v.y, v.z, v.w}}; }

// ---------------------------------------------------------------------------
// Dtype rules: the element, how many a slice holds, element <-> slice, and what
// one slice adds to {NaN count, sum cur^2, sum d^2}.
// ---------------------------------------------------------------------------
// bf16 / fp16; R = BF16Pk / F16Pk (common.hpp): two elements per 32-bit word
template <class R>
struct CvHalf {
  typedef unsigned short elem;
  static constexpr int kPer = 8;
  static constexpr bool kF64 = false;
  __device__ static void put(CvSlice& v, int i, elem e) { v.w[i >> 1] |= static_cast<unsigned int>(e) << (16 * (i & 1)); }
  __device__ static elem get(const CvSlice& v, int i) { return static_cast<elem>(v.w[i >> 1] >> (16 * (i & 1))); }
  template <bool HAS>
  __device__ static void add(const CvSlice& c, const CvSlice& s, int& nans, double& a_cur, double& a_d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x2 x = R::unpack(c.w[k]);
      nans += static_cast<int>(x.x != x.x) + static_cast<int>(x.y != x.y);
      const double p = x.x, q = x.y;  // the fp64 square of a widened 16-bit value is exact
      a_cur = __builtin_fma(p, p, a_cur);
      a_cur = __builtin_fma(q, q, a_cur);
      if constexpr (HAS) {
        // rT(f32(cur) - f32(snap)): ATen's opmath subtraction rounded to the model's type, widened exactly
        const f32x2 d = R::unpack(R::pack(opaque2(x - R::unpack(s.w[k]))));
        const double dp = d.x, dq = d.y;
        a_d = __builtin_fma(dp, dp, a_d);
        a_d = __builtin_fma(dq, dq, a_d);
      }
    }
  }
  // rT(x) as a double
  __device__ static double rt(float x) { return static_cast<double>(R::unpack(R::pack(opaque2(f32x2{x, 0.f}))).x); }
};

struct CvF64 {
  typedef double elem;
  static constexpr int kPer = 2;
  static constexpr bool kF64 = true;
  __device__ static void put(CvSlice& v, int i, elem e) {
    const uint64_t u = __builtin_bit_cast(uint64_t, e);
    v.w[2 * i] = static_cast<unsigned int>(u);
    v.w[2 * i + 1] = static_cast<unsigned int>(u >> 32);
  }
  __device__ static elem get(const CvSlice& v, int i) {
    return __builtin_bit_cast(double, (static_cast<uint64_t>(v.w[2 * i + 1]) << 32) | v.w[2 * i]);
  }
  template <bool HAS>
  __device__ static void add(const CvSlice& c, const CvSlice& s, int& nans, double& a_cur, double& a_d) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double x = get(c, k);
      nans += static_cast<int>(x != x);
      a_cur = __builtin_fma(x, x, a_cur);
      if constexpr (HAS) {
        const double d = x - get(s, k);  // fp64 difference, as the reference forms it
        a_d = __builtin_fma(d, d, a_d);
      }
    }
  }
};

// elements [col, col + kPer) of a unit of n columns of the model's tensor: one
// 16-B nontemporal load when the tensor is 16-B aligned and the slice is
// whole, else element by element (columns past n read as 0)
template <class T, bool VEC>
__device__ __forceinline__ CvSlice load_cur(const typename T::elem* p, int col, int n) {
  if (VEC && col + T::kPer <= n) return cv_slice(__builtin_nontemporal_load(to_global<u32x4>(p + col)));
  const gptr<typename T::elem> q = to_global<typename T::elem>(p);
  CvSlice v{{0u, 0u, 0u, 0u}};
#pragma unroll
  for (int i = 0; i < T::kPer; ++i)
    if (col + i < n) T::put(v, i, __builtin_nontemporal_load(q + col + i));
  return v;
}

// the snapshot's slice (16-B aligned: key offsets are multiples of 16 B)
template <class T>
__device__ __forceinline__ CvSlice load_snap(const typename T::elem* p, int col, int n) {
  if (col + T::kPer <= n) return cv_slice(*reinterpret_cast<const u32x4*>(p + col));
  CvSlice v{{0u, 0u, 0u, 0u}};
#pragma unroll
  for (int i = 0; i < T::kPer - 1; ++i)
    if (col + i < n) T::put(v, i, p[col + i]);
  return v;
}

template <class T>
__device__ __forceinline__ void store_snap(typename T::elem* p, int col, int n, const CvSlice& a) {
  if (col + T::kPer <= n) {
    *reinterpret_cast<u32x4*>(p + col) = u32x4{a.w[0], a.w[1], a.w[2], a.w[3]};
  } else {
#pragma unroll
    for (int i = 0; i < T::kPer - 1; ++i)
      if (col + i < n) p[col + i] = T::get(a, i);
  }
}

// one unit: this thread's kCvC slices; acc = {NaN count, sum cur^2, sum d^2}
template <class T, bool HAS, bool VEC>
__device__ __forceinline__ void client_unit(const typename T::elem* __restrict__ cur,
                                            typename T::elem* __restrict__ snap, int n, double (&acc)[kCvStats]) {
  CvSlice cv[kCvC], sv[kCvC];
#pragma unroll
  for (int s = 0; s < kCvC; ++s)
    cv[s] = load_cur<T, VEC>(cur, T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock), n);
#pragma unroll
  for (int s = 0; s < kCvC; ++s) {
    if constexpr (HAS)
      sv[s] = load_snap<T>(snap, T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock), n);
    else
      sv[s] = CvSlice{{0u, 0u, 0u, 0u}};
  }
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCvC; ++s) {
    T::template add<HAS>(cv[s], sv[s], nans, acc[1], acc[2]);
    store_snap<T>(snap, T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock), n, cv[s]);
  }
  acc[0] = static_cast<double>(nans);
}

// partials[i][u]: workgroup u's NaN count (i = 0), sum cur^2 (1), sum d^2 (2)
template <class T, bool HAS>
__global__ __launch_bounds__(kBlock) void clientvec_stats_kernel(const ClientKey* __restrict__ keys, int64_t n_keys,
                                                                 typename T::elem* __restrict__ snap,
                                                                 double* __restrict__ partials, int64_t units) {
  constexpr int64_t span = kCvUnitBytes / static_cast<int64_t>(sizeof(typename T::elem));
  __shared__ double red[kCvStats][kBlock / 64];
  const int64_t u = blockIdx.x;
  const int64_t j = wave_search_last_le([&](int64_t x) { return keys[x].unit_start; }, n_keys, u);
  const ClientKey key = keys[j];
  const int64_t c0 = (u - key.unit_start) * span;
  const int n = static_cast<int>(key.numel - c0 < span ? key.numel - c0 : span);
  const typename T::elem* cur = reinterpret_cast<const typename T::elem*>(key.ptr) + c0;
  typename T::elem* sn = snap + key.snap_offset + c0;
  double acc[kCvStats] = {0.0, 0.0, 0.0};
  if ((key.ptr & 15) == 0)
    client_unit<T, HAS, true>(cur, sn, n, acc);
  else
    client_unit<T, HAS, false>(cur, sn, n, acc);
#pragma unroll
  for (int i = 0; i < kCvStats; ++i) {
    const double w = wave_sum_dpp(acc[i]);
    if ((threadIdx.x & 63u) == 0) red[i][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < kCvStats) {
    double s = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
    partials[static_cast<int64_t>(threadIdx.x) * units + u] = s;
  }
}

// stats[i] = sum over the workgroups' partials in a fixed order; stats[3] = 0
__global__ __launch_bounds__(kBlock) void clientvec_finalize_kernel(const double* __restrict__ partials, int64_t units,
                                                                    double* __restrict__ stats) {
  __shared__ double red[kBlock];
  for (int i = 0; i < kCvStats; ++i) {
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

// client.py:78-84 on the device in the model's type; `state` holds values of
// T exactly.  `not x or tmp > x` (:79, :83)
__device__ __forceinline__ void track_update(double* __restrict__ x, double* __restrict__ has, double tmp) {
  const double cur = *x;
  if (*has == 0.0 || cur == 0.0 || tmp > cur) *x = tmp;
  *has = 1.0;
}

// Every fp32 operation is formed in fp64 from fp32 operands and rounded once
// to fp32 (for sqrt, a quotient and a product of fp32 values that is the
// correctly rounded fp32 result, 53 >= 2 * 24 + 2), then rounded to T as ATen
// casts its opmath result.  fp64 models: the same operations in fp64.
template <class T>
__global__ __launch_bounds__(64) void clientvec_track_kernel(double* __restrict__ state,
                                                             const double* __restrict__ w_stats,
                                                             const double* __restrict__ g_stats, double abs_dloss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double rho_tmp, beta_tmp;
  if constexpr (T::kF64) {
    const double n_w = __builtin_sqrt(w_stats[2]);  // norm(w - last_w)
    const double n_g = __builtin_sqrt(g_stats[2]);  // norm(grads - last_grads)
    const double recip = 1.0 / n_w;
    rho_tmp = recip * abs_dloss;
    beta_tmp = n_g / n_w;
  } else {
    const double n_w = T::rt(static_cast<float>(__builtin_sqrt(w_stats[2])));
    const double n_g = T::rt(static_cast<float>(__builtin_sqrt(g_stats[2])));
    const double recip = T::rt(static_cast<float>(1.0 / n_w));
    const double dl = static_cast<double>(static_cast<float>(abs_dloss));
    rho_tmp = T::rt(static_cast<float>(recip * dl));
    beta_tmp = T::rt(static_cast<float>(n_g / n_w));
  }
  track_update(state + 0, state + 2, rho_tmp);
  track_update(state + 1, state + 3, beta_tmp);
}

int64_t span_of(int64_t elem_size) { return elem_size == 2 || elem_size == 8 ? kCvUnitBytes / elem_size : 0; }

int zero_stats(const char* what, double* stats, hipStream_t s) {
  if (!is_device_memory(stats)) return cv_error(FEDAVG_EINVAL, "%s: stats must be device memory", what);
  const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(double), s);
  if (e == hipSuccess) return FEDAVG_OK;
  (void)hipGetLastError();
  return cv_error(-static_cast<int>(e), "%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
}

template <class T>
int client_stats_vec(const char* what, const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                     int64_t n_keys, typename T::elem* snap, int64_t P, int has_snap, double* partials,
                     int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                     void* stream) {
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  constexpr int64_t span = kCvUnitBytes / es;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0 || P < 0) return cv_error(FEDAVG_EINVAL, "%s: negative n_keys or P", what);
  if (!stats) return cv_error(FEDAVG_EINVAL, "%s: null stats", what);
  if (P == 0 || n_keys == 0) return zero_stats(what, stats, s);
  if (!cur_ptrs || !key_numel || !key_offset || !snap || !partials || !host_ws || !dev_ws)
    return cv_error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = fedavg_client_stats_vec_workspace(n_keys);
  if (ws_bytes < need_ws) return cv_error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j) {
    const int64_t n = key_numel[j], off = key_offset[j];
    if (n < 0 || off < 0 || off > P || n > P - off)
      return cv_error(FEDAVG_EINVAL, "%s: key %lld lies outside the snapshot of %lld elements", what, (long long)j,
                      (long long)P);
    if (n > 0 && (cur_ptrs[j] == 0 || (cur_ptrs[j] & (es - 1)) != 0))
      return cv_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                      (long long)j, (long long)es);
    units += (n + span - 1) / span;
  }
  if (units > INT32_MAX) return cv_error(FEDAVG_EINVAL, "%s: too many units", what);
  const int64_t need_parts = kCvStats * units;
  if (partial_elems < need_parts)
    return cv_error(FEDAVG_EINVAL, "%s: partials need %lld doubles", what, (long long)need_parts);
  if (!aligned16(snap)) return cv_error(FEDAVG_EALIGN, "%s: snap must be 16-B aligned", what);
  for (int64_t j = 0; j < n_keys; ++j)
    if (key_offset[j] % (16 / es))
      return cv_error(FEDAVG_EALIGN, "%s: key %lld: snapshot offset must be a multiple of %lld elements", what,
                      (long long)j, (long long)(16 / es));
  if (!aligned16(host_ws) || !aligned16(dev_ws) || (reinterpret_cast<uintptr_t>(partials) & 7u) ||
      (reinterpret_cast<uintptr_t>(stats) & 7u))
    return cv_error(FEDAVG_EALIGN, "%s: workspaces must be 16-B, partials and stats 8-B aligned", what);
  if (units == 0) return zero_stats(what, stats, s);
  if (!is_pinned_host_memory(host_ws)) return cv_error(FEDAVG_EINVAL, "%s: host_ws is not pinned host memory", what);
  if (!is_device_memory(dev_ws) || !is_device_memory(snap) || !is_device_memory(partials) || !is_device_memory(stats))
    return cv_error(FEDAVG_EINVAL, "%s: dev_ws, snap, partials and stats must be device memory", what);
  // a host address would fault the kernel: spot check of the first and last
  // tensor (the Python layer checks every tensor's device)
  auto* hk = static_cast<ClientKey*>(host_ws);
  int64_t u0 = 0, first = -1, last = -1;
  for (int64_t j = 0; j < n_keys; ++j) {
    hk[j] = ClientKey{cur_ptrs[j], key_numel[j], key_offset[j], u0};
    u0 += (key_numel[j] + span - 1) / span;
    if (key_numel[j] > 0) {
      if (first < 0) first = j;
      last = j;
    }
  }
  if (!is_device_memory(reinterpret_cast<const void*>(cur_ptrs[first])) ||
      !is_device_memory(reinterpret_cast<const void*>(cur_ptrs[last])))
    return cv_error(FEDAVG_EINVAL, "%s: the tensors must be device memory", what);
  const hipError_t e = hipMemcpyAsync(dev_ws, host_ws, static_cast<size_t>(need_ws), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return cv_error(-static_cast<int>(e), "%s: hipMemcpyAsync failed: %s", what, hipGetErrorString(e));
  }
  const auto* keys = static_cast<const ClientKey*>(dev_ws);
  if (has_snap)
    hipLaunchKernelGGL((clientvec_stats_kernel<T, true>), dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, snap, partials, units);
  else
    hipLaunchKernelGGL((clientvec_stats_kernel<T, false>), dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, snap, partials, units);
  const int rc = cv_launch_status(what);
  if (rc) return rc;
  hipLaunchKernelGGL(clientvec_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  return cv_launch_status(what);
}

template <class T>
int client_track_vec(const char* what, double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                     void* stream) {
  if (!state || !w_stats || !g_stats) return cv_error(FEDAVG_EINVAL, "%s: null argument", what);
  if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(w_stats) |
       reinterpret_cast<uintptr_t>(g_stats)) & 7u)
    return cv_error(FEDAVG_EALIGN, "%s: records must be 8-B aligned", what);
  if (!is_device_memory(state) || !is_device_memory(w_stats) || !is_device_memory(g_stats))
    return cv_error(FEDAVG_EINVAL, "%s: state and records must be device memory", what);
  hipLaunchKernelGGL(clientvec_track_kernel<T>, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, w_stats,
                     g_stats, abs_dloss);
  return cv_launch_status(what);
}

}  // namespace

extern "C" {

int fedavg_clientvec_abi_version(void) { return 1; }

const char* fedavg_clientvec_last_error(void) { return g_cv_err.c_str(); }

int64_t fedavg_client_stats_vec_span(int64_t elem_size) { return span_of(elem_size); }

int64_t fedavg_client_stats_vec_workspace(int64_t n_keys) {
  return n_keys > 0 ? n_keys * static_cast<int64_t>(sizeof(ClientKey)) : 0;
}

int64_t fedavg_client_stats_vec_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  const int64_t span = span_of(elem_size);
  if (!key_numel || n_keys <= 0 || span == 0) return 0;
  int64_t units = 0;
  for (int64_t j = 0; j < n_keys; ++j)
    if (key_numel[j] > 0) units += (key_numel[j] + span - 1) / span;
  return kCvStats * units;
}

int fedavg_client_stats_bf16(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                             int64_t n_keys, uint16_t* snap, int64_t P, int has_snap, double* partials,
                             int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                             void* stream) {
  return client_stats_vec<CvHalf<BF16Pk>>("fedavg_client_stats_bf16", cur_ptrs, key_numel, key_offset, n_keys, snap, P,
                                          has_snap, partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_stats_f16(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, uint16_t* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream) {
  return client_stats_vec<CvHalf<F16Pk>>("fedavg_client_stats_f16", cur_ptrs, key_numel, key_offset, n_keys, snap, P,
                                         has_snap, partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_stats_f64(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, double* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream) {
  return client_stats_vec<CvF64>("fedavg_client_stats_f64", cur_ptrs, key_numel, key_offset, n_keys, snap, P, has_snap,
                                 partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_track_bf16(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                             void* stream) {
  return client_track_vec<CvHalf<BF16Pk>>("fedavg_client_track_bf16", state, w_stats, g_stats, abs_dloss, stream);
}

int fedavg_client_track_f16(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                            void* stream) {
  return client_track_vec<CvHalf<F16Pk>>("fedavg_client_track_f16", state, w_stats, g_stats, abs_dloss, stream);
}

int fedavg_client_track_f64(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                            void* stream) {
  return client_track_vec<CvF64>("fedavg_client_track_f64", state, w_stats, g_stats, abs_dloss, stream);
}

}  // extern "C"
