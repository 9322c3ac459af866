// fedavg_client_step.hip -- libfedavg_amd_clientstep.so (include/
// fedavg_amd_clientstep.h): the client's plain SGD step (client.py:74) and the
// weight statistics of :76-82 in one pass, for fp32, bf16, fp16 and fp64
// models.
//
// After optimizer.step() the statistics pass of fedavg_client.hip /
// fedavg_client_vec.hip reads the weights again, next to a snapshot of the
// weights before the step, only to form norm(w - last_w) and norm(w).  The
// step already holds both values of every element in registers, so here one
// kernel reads w and g, forms
//     w' = rT(fma(alpha, g, w))          form 1 (one rounding in opmath)
//     w' = rT(w + fl(alpha * g))         form 0 (product and sum rounded apart)
//     d  = rT(w' - w)                    the difference in the model's type (:78)
//     count of isnan(w'), sum w'^2, sum d^2      (squares and sums in fp64)
// and stores w': 12 B per fp32 element instead of 24, no snapshot.  The unit
// is -ffp-contract=off (and common.hpp pins it), so form 1 is an explicit
// __builtin_fma[f] and form 0 stays unfused; which one equals torch's bits is
// the caller's finding (client_stats.sgd_form).
//
// The pass has the shape of those two: a staged key table (client_step_plan.hpp),
// one workgroup of 256 threads per unit of 16 KiB of a tensor, wave search for
// the unit's key, a thread owning 4 slices of 16 B (slice s at byte
// 16 * (tid + 256 s)) of w and of g, its 4 + 4 loads issued before the first
// use, g nontemporally (read once; backward leaves a fresh tensor every
// iteration).  Each side of a key is read 16 B at a time when its address is
// 16-B aligned, else element by element into the same slices, so every path
// adds the same values in the same order; columns past the key's end count as
// nothing and are never stored.  Wave sums by DPP, the 4 waves added in wave
// order, three fp64 partials per workgroup, a one-workgroup finalize: no
// floating-point atomics, the same bits run to run.
#include "common.hpp"

#include "client_step_plan.hpp"
#include "fedavg_amd_clientstep.h"

namespace {
using namespace fedavg_impl;

thread_local ErrorState g_cs_err;

int cs_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cs_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int cs_launch_status(const char* what) { return launch_status(g_cs_err, what); }

static_assert(kStepUnitBytes == static_cast<int64_t>(kBlock) * 4 * 16, "client_step_plan.hpp plans for this workgroup");
constexpr int kCsC = 4;  // 16-B slices per thread

template <typename T>
using gptr = __attribute__((address_space(1))) const T*;

template <typename T>
__device__ __forceinline__ gptr<T> to_global(const void* p) {
  return (gptr<T>)(reinterpret_cast<uintptr_t>(p));
}

template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T* to_global_mut(void* p) {
  return (__attribute__((address_space(1))) T*)(reinterpret_cast<uintptr_t>(p));
}

// 16 B of a tensor as they lie in memory
struct CsSlice {
  unsigned int w[4];
};

__device__ __forceinline__ CsSlice cs_slice(u32x4 v) { return CsSlice{{v.x, v.y, v.z, v.w}}; }

__device__ __forceinline__ void add_sq(double& acc, double x) { acc = __builtin_fma(x, x, acc); }

// ---------------------------------------------------------------------------
// Dtype rules: the element, the opmath type, how many elements a slice holds,
// element <-> slice, and the step of one slice: out = w', {NaN count, sum
// w'^2, sum d^2} += its first `live` elements (the others are columns past
// the key's end: whatever alpha makes of their zeros counts as nothing).
// ---------------------------------------------------------------------------
struct CsF32 {
  typedef float elem;
  typedef float op;
  static constexpr int kPer = 4;
  __device__ static void put(CsSlice& v, int i, elem e) { v.w[i] = __float_as_uint(e); }
  __device__ static elem get(const CsSlice& v, int i) { return __uint_as_float(v.w[i]); }
  template <int FORM>
  __device__ static void step(const CsSlice& c, const CsSlice& g, op alpha, int live, CsSlice& out, int& nans,
                              double& a_w, double& a_d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float w = __uint_as_float(c.w[k]), x = __uint_as_float(g.w[k]);
      float wn;
      if constexpr (FORM)
        wn = __builtin_fmaf(alpha, x, w);
      else
        wn = w + alpha * x;
      out.w[k] = __float_as_uint(wn);
      const bool on = k < live;
      const float d = wn - w;  // fp32 difference, as w - last_w at :78
      nans += static_cast<int>(on && wn != wn);
      add_sq(a_w, on ? static_cast<double>(wn) : 0.0);  // the fp64 square of an fp32 value is exact
      add_sq(a_d, on ? static_cast<double>(d) : 0.0);
    }
  }
};

// bf16 / fp16; R = BF16Pk / F16Pk (common.hpp): two elements per 32-bit word
template <class R>
struct CsHalf {
  typedef unsigned short elem;
  typedef float op;
  static constexpr int kPer = 8;
  __device__ static void put(CsSlice& v, int i, elem e) { v.w[i >> 1] |= static_cast<unsigned int>(e) << (16 * (i & 1)); }
  __device__ static elem get(const CsSlice& v, int i) { return static_cast<elem>(v.w[i >> 1] >> (16 * (i & 1))); }
  template <int FORM>
  __device__ static void step(const CsSlice& c, const CsSlice& g, op alpha, int live, CsSlice& out, int& nans,
                              double& a_w, double& a_d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const f32x2 w = R::unpack(c.w[k]), x = R::unpack(g.w[k]);
      f32x2 wn;
      if constexpr (FORM)
        wn = f32x2{__builtin_fmaf(alpha, x.x, w.x), __builtin_fmaf(alpha, x.y, w.y)};
      else
        wn = w + alpha * x;
      out.w[k] = R::pack(opaque2(wn));  // ATen's opmath result rounded to the model's type
      const f32x2 q = R::unpack(out.w[k]);
      const f32x2 d = R::unpack(R::pack(opaque2(q - w)));  // rT(f32(w') - f32(w)), widened exactly
      const bool on0 = 2 * k < live, on1 = 2 * k + 1 < live;
      nans += static_cast<int>(on0 && q.x != q.x) + static_cast<int>(on1 && q.y != q.y);
      add_sq(a_w, on0 ? static_cast<double>(q.x) : 0.0);  // the fp64 square of a widened 16-bit value is exact
      add_sq(a_w, on1 ? static_cast<double>(q.y) : 0.0);
      add_sq(a_d, on0 ? static_cast<double>(d.x) : 0.0);
      add_sq(a_d, on1 ? static_cast<double>(d.y) : 0.0);
    }
  }
};

struct CsF64 {
  typedef double elem;
  typedef double op;
  static constexpr int kPer = 2;
  __device__ static void put(CsSlice& v, int i, elem e) {
    const uint64_t u = __builtin_bit_cast(uint64_t, e);
    v.w[2 * i] = static_cast<unsigned int>(u);
    v.w[2 * i + 1] = static_cast<unsigned int>(u >> 32);
  }
  __device__ static elem get(const CsSlice& v, int i) {
    return __builtin_bit_cast(double, (static_cast<uint64_t>(v.w[2 * i + 1]) << 32) | v.w[2 * i]);
  }
  template <int FORM>
  __device__ static void step(const CsSlice& c, const CsSlice& g, op alpha, int live, CsSlice& out, int& nans,
                              double& a_w, double& a_d) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double w = get(c, k), x = get(g, k);
      double wn;
      if constexpr (FORM)
        wn = __builtin_fma(alpha, x, w);
      else
        wn = w + alpha * x;
      put(out, k, wn);
      const bool on = k < live;
      const double d = wn - w;  // fp64 difference, as the reference forms it
      nans += static_cast<int>(on && wn != wn);
      add_sq(a_w, on ? wn : 0.0);
      add_sq(a_d, on ? d : 0.0);
    }
  }
};

// elements [col, col + kPer) of a unit of n columns: one 16-B load when the
// side is 16-B aligned and the slice is whole, else element by element
// (columns past n read as 0); NT: nontemporal (the gradients)
template <class T, bool VEC, bool NT>
__device__ __forceinline__ CsSlice load_slice(const typename T::elem* p, int col, int n) {
  if (VEC && col + T::kPer <= n) {
    const gptr<u32x4> q = to_global<u32x4>(p + col);
    return cs_slice(NT ? __builtin_nontemporal_load(q) : *q);
  }
  const gptr<typename T::elem> q = to_global<typename T::elem>(p);
  CsSlice v{{0u, 0u, 0u, 0u}};
#pragma unroll
  for (int i = 0; i < T::kPer; ++i)
    if (col + i < n) T::put(v, i, NT ? __builtin_nontemporal_load(q + col + i) : q[col + i]);
  return v;
}

// w'[col, col + kPer) back: a whole slice of a 16-B aligned tensor in one
// store, anything else by guarded element stores (nothing at or past n)
template <class T, bool VEC>
__device__ __forceinline__ void store_slice(typename T::elem* p, int col, int n, const CsSlice& a) {
  if (VEC && col + T::kPer <= n) {
    *to_global_mut<u32x4>(p + col) = u32x4{a.w[0], a.w[1], a.w[2], a.w[3]};
  } else {
    const auto q = to_global_mut<typename T::elem>(p);
#pragma unroll
    for (int i = 0; i < T::kPer; ++i)
      if (col + i < n) q[col + i] = T::get(a, i);
  }
}

// one unit: this thread's kCsC slices; acc = {NaN count, sum w'^2, sum d^2}
template <class T, int FORM, bool WVEC, bool GVEC>
__device__ __forceinline__ void step_unit(typename T::elem* w, const typename T::elem* g, int n, typename T::op alpha,
                                          double (&acc)[kStepStats]) {
  CsSlice wv[kCsC], gv[kCsC];
#pragma unroll
  for (int s = 0; s < kCsC; ++s)
    wv[s] = load_slice<T, WVEC, false>(w, T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock), n);
#pragma unroll
  for (int s = 0; s < kCsC; ++s)
    gv[s] = load_slice<T, GVEC, true>(g, T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock), n);
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCsC; ++s) {
    const int col = T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock);
    CsSlice out;
    T::template step<FORM>(wv[s], gv[s], alpha, n - col, out, nans, acc[1], acc[2]);
    store_slice<T, WVEC>(w, col, n, out);
  }
  acc[0] = static_cast<double>(nans);
}

// partials[i][u]: workgroup u's NaN count (i = 0), sum w'^2 (1), sum d^2 (2)
template <class T, int FORM>
__global__ __launch_bounds__(kBlock) void client_sgd_step_kernel(const StepKey* __restrict__ keys, int64_t n_keys,
                                                                 typename T::op alpha, double* __restrict__ partials,
                                                                 int64_t units) {
  constexpr int64_t span = kStepUnitBytes / static_cast<int64_t>(sizeof(typename T::elem));
  __shared__ double red[kStepStats][kBlock / 64];
  const int64_t u = blockIdx.x;
  const int64_t j = wave_search_last_le([&](int64_t x) { return keys[x].unit_start; }, n_keys, u);
  const StepKey key = keys[j];
  const int64_t c0 = (u - key.unit_start) * span;
  const int n = static_cast<int>(key.numel - c0 < span ? key.numel - c0 : span);
  typename T::elem* w = reinterpret_cast<typename T::elem*>(key.w) + c0;
  const typename T::elem* g = reinterpret_cast<const typename T::elem*>(key.g) + c0;
  double acc[kStepStats] = {0.0, 0.0, 0.0};
  // a unit starts a multiple of 16 KiB into its tensor: the tensor's alignment is the unit's
  const bool wvec = (key.w & 15) == 0, gvec = (key.g & 15) == 0;
  if (wvec && gvec)
    step_unit<T, FORM, true, true>(w, g, n, alpha, acc);
  else if (wvec)
    step_unit<T, FORM, true, false>(w, g, n, alpha, acc);
  else if (gvec)
    step_unit<T, FORM, false, true>(w, g, n, alpha, acc);
  else
    step_unit<T, FORM, false, false>(w, g, n, alpha, acc);
#pragma unroll
  for (int i = 0; i < kStepStats; ++i) {
    const double s = wave_sum_dpp(acc[i]);
    if ((threadIdx.x & 63u) == 0) red[i][threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x < kStepStats) {
    double s = red[threadIdx.x][0];
#pragma unroll
    for (int v = 1; v < kBlock / 64; ++v) s += red[threadIdx.x][v];
    partials[static_cast<int64_t>(threadIdx.x) * units + u] = s;
  }
}

// stats[i] = sum over the workgroups' partials in a fixed order; stats[3] = 0
__global__ __launch_bounds__(kBlock) void client_sgd_step_finalize_kernel(const double* __restrict__ partials,
                                                                          int64_t units, double* __restrict__ stats) {
  __shared__ double red[kBlock];
  for (int i = 0; i < kStepStats; ++i) {
    double s = 0.0;
    for (int64_t v = threadIdx.x; v < units; v += kBlock) s += partials[i * units + v];
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

int zero_stats(const char* what, double* stats, hipStream_t s) {
  if (!is_device_memory(stats)) return cs_error(FEDAVG_EINVAL, "%s: stats must be device memory", what);
  const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(double), s);
  if (e == hipSuccess) return FEDAVG_OK;
  (void)hipGetLastError();
  return cs_error(-static_cast<int>(e), "%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
}

template <class T>
int client_sgd_step(const char* what, const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                    int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems, double* stats,
                    void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  constexpr int64_t span = kStepUnitBytes / es;
  static_assert(span == step_span(es), "client_step_plan.hpp cuts the same units");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0) return cs_error(FEDAVG_EINVAL, "%s: negative n_keys", what);
  if (!stats) return cs_error(FEDAVG_EINVAL, "%s: null stats", what);
  if (form != 0 && form != 1) return cs_error(FEDAVG_EMODE, "%s: form %d is neither 0 nor 1", what, form);
  if (n_keys == 0) return zero_stats(what, stats, s);
  if (!w_ptrs || !g_ptrs || !key_numel || !partials || !host_ws || !dev_ws)
    return cs_error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = step_workspace(n_keys);
  if (ws_bytes < need_ws) return cs_error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  for (int64_t j = 0; j < n_keys; ++j) {
    const int64_t n = key_numel[j];
    if (n < 0) return cs_error(FEDAVG_EINVAL, "%s: key %lld: negative size", what, (long long)j);
    if (n > 0 && (w_ptrs[j] == 0 || g_ptrs[j] == 0 || ((w_ptrs[j] | g_ptrs[j]) & (es - 1)) != 0))
      return cs_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                      (long long)j, (long long)es);
  }
  const int64_t units = step_units(key_numel, n_keys, span);
  if (units > INT32_MAX) return cs_error(FEDAVG_EINVAL, "%s: too many units", what);
  const int64_t need_parts = kStepStats * units;
  if (partial_elems < need_parts)
    return cs_error(FEDAVG_EINVAL, "%s: partials need %lld doubles", what, (long long)need_parts);
  if (!aligned16(host_ws) || !aligned16(dev_ws) || (reinterpret_cast<uintptr_t>(partials) & 7u) ||
      (reinterpret_cast<uintptr_t>(stats) & 7u))
    return cs_error(FEDAVG_EALIGN, "%s: workspaces must be 16-B, partials and stats 8-B aligned", what);
  if (units == 0) return zero_stats(what, stats, s);
  if (!is_pinned_host_memory(host_ws)) return cs_error(FEDAVG_EINVAL, "%s: host_ws is not pinned host memory", what);
  if (!is_device_memory(dev_ws) || !is_device_memory(partials) || !is_device_memory(stats))
    return cs_error(FEDAVG_EINVAL, "%s: dev_ws, partials and stats must be device memory", what);
  const StepFill f = step_fill(static_cast<StepKey*>(host_ws), w_ptrs, g_ptrs, key_numel, n_keys, span);
  // a host address would fault the kernel: spot check of the first and last
  // tensor of each side (the Python layer checks every tensor's device)
  for (const int64_t* side : {w_ptrs, g_ptrs})
    if (!is_device_memory(reinterpret_cast<const void*>(side[f.first])) ||
        !is_device_memory(reinterpret_cast<const void*>(side[f.last])))
      return cs_error(FEDAVG_EINVAL, "%s: the tensors must be device memory", what);
  const hipError_t e = hipMemcpyAsync(dev_ws, host_ws, static_cast<size_t>(need_ws), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return cs_error(-static_cast<int>(e), "%s: hipMemcpyAsync failed: %s", what, hipGetErrorString(e));
  }
  const auto* keys = static_cast<const StepKey*>(dev_ws);
  const typename T::op alpha = static_cast<typename T::op>(-lr);  // ATen: the scalar rounded once to opmath
  if (form)
    hipLaunchKernelGGL((client_sgd_step_kernel<T, 1>), dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, alpha, partials, units);
  else
    hipLaunchKernelGGL((client_sgd_step_kernel<T, 0>), dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys,
                       n_keys, alpha, partials, units);
  const int rc = cs_launch_status(what);
  if (rc) return rc;
  hipLaunchKernelGGL(client_sgd_step_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  return cs_launch_status(what);
}

}  // namespace

extern "C" {

int fedavg_clientstep_abi_version(void) { return 1; }

const char* fedavg_clientstep_last_error(void) { return g_cs_err.c_str(); }

int64_t fedavg_client_step_span(int64_t elem_size) { return step_span(elem_size); }

int64_t fedavg_client_step_workspace(int64_t n_keys) { return step_workspace(n_keys); }

int64_t fedavg_client_step_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  const int64_t span = step_span(elem_size);
  if (!key_numel || n_keys <= 0 || span == 0) return 0;
  return kStepStats * step_units(key_numel, n_keys, span);
}

int fedavg_client_sgd_step_f32(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return client_sgd_step<CsF32>("fedavg_client_sgd_step_f32", w_ptrs, g_ptrs, key_numel, n_keys, lr, form, partials,
                                partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_sgd_step_bf16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                                double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return client_sgd_step<CsHalf<BF16Pk>>("fedavg_client_sgd_step_bf16", w_ptrs, g_ptrs, key_numel, n_keys, lr, form,
                                         partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_sgd_step_f16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return client_sgd_step<CsHalf<F16Pk>>("fedavg_client_sgd_step_f16", w_ptrs, g_ptrs, key_numel, n_keys, lr, form,
                                        partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

int fedavg_client_sgd_step_f64(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return client_sgd_step<CsF64>("fedavg_client_sgd_step_f64", w_ptrs, g_ptrs, key_numel, n_keys, lr, form, partials,
                                partial_elems, stats, host_ws, dev_ws, ws_bytes, stream);
}

}  // extern "C"
