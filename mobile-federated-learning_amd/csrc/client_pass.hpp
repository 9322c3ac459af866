// client_pass.hpp -- the one pass behind the client libraries' kernels: the
// statistics of fp32 models (fedavg_client.hip), of bf16 / fp16 / fp64 models
// (fedavg_client_vec.hip), the SGD and Adam steps fused with the weight
// statistics (fedavg_client_step.hip, fedavg_client_adam.hip) and their gated
// forms (fedavg_client_loop.hip).  Each of those files keeps its __global__
// entry points and its C ABI; the pass is here, once, and the steps' dtype
// rules are in client_step_rules.hpp / client_adam_rules.hpp, once.
//
// The host stages a table of 32 B per key (client_pass_plan.hpp) and launches
// one workgroup of 256 threads per unit of 16 KiB of a tensor.  The workgroup
// finds its key by a wave search of the table; a thread owns 4 slices of 16 B
// (slice s at byte 16 * (tid + 256 s)) of each of the key's two sides, its
// 4 + 4 loads issued before the first use.  A side is read 16 B at a time when
// it is 16-B aligned, else element by element into the same slices, so every
// path adds the same values in the same order; columns past the key's end read
// as zero and are never stored.  A dtype rule says what one slice adds to
// {NaN count, sum x^2, sum d^2}, squares and sums in fp64.  Every workgroup
// writes its three partials (wave sums by DPP, the 4 waves added in wave
// order) and a one-workgroup finalize adds them in a fixed order: no
// floating-point atomics, the same bits run to run.
//
// The sides, and how each is reached (address space and cache policy are part
// of the pass's speed):
//   statistics: the model's tensor    global, nontemporal (read once)
//               the snapshot          generic pointer, plain; always 16-B aligned
//   step:       w                     global, plain, stored back the same way
//               g                     global, nontemporal (backward leaves a fresh tensor)
#pragma once

#include "common.hpp"

#include "client_pass_plan.hpp"

namespace fedavg_impl {

constexpr int kCliC = 4;  // 16-B slices per thread
static_assert(kClientUnitBytes == static_cast<int64_t>(kBlock) * kCliC * 16, "client_pass_plan.hpp plans for this workgroup");

template <typename X>
__device__ __forceinline__ __attribute__((address_space(1))) const X* to_global(const X* p) {
  return (__attribute__((address_space(1))) const X*)(reinterpret_cast<uintptr_t>(p));
}

template <typename X>
__device__ __forceinline__ __attribute__((address_space(1))) X* to_global(X* p) {
  return (__attribute__((address_space(1))) X*)(reinterpret_cast<uintptr_t>(p));
}

// 16 B of a tensor as they lie in memory
struct CliSlice {
  unsigned int w[4];
};

__device__ __forceinline__ CliSlice cli_slice(u32x4 v) { return CliSlice{{v.x, v.y, v.z, v.w}}; }

// acc += x^2 in fp64, one rounding
__device__ __forceinline__ void add_sq(double& acc, double x) { acc = __builtin_fma(x, x, acc); }

// The element of ES bytes, how many a slice holds, element <-> slice (put
// into a zeroed slice).  A dtype rule derives from one of these.
template <int ES>
struct CliElem;

template <>
struct CliElem<4> {
  typedef float elem;
  static constexpr int kPer = 4;
  __device__ static void put(CliSlice& v, int i, elem e) { v.w[i] = __float_as_uint(e); }
  __device__ static elem get(const CliSlice& v, int i) { return __uint_as_float(v.w[i]); }
};

template <>
struct CliElem<2> {
  typedef unsigned short elem;
  static constexpr int kPer = 8;
  __device__ static void put(CliSlice& v, int i, elem e) { v.w[i >> 1] |= static_cast<unsigned int>(e) << (16 * (i & 1)); }
  __device__ static elem get(const CliSlice& v, int i) { return static_cast<elem>(v.w[i >> 1] >> (16 * (i & 1))); }
};

template <>
struct CliElem<8> {
  typedef double elem;
  static constexpr int kPer = 2;
  __device__ static void put(CliSlice& v, int i, elem e) {
    const uint64_t u = __builtin_bit_cast(uint64_t, e);
    v.w[2 * i] = static_cast<unsigned int>(u);
    v.w[2 * i + 1] = static_cast<unsigned int>(u >> 32);
  }
  __device__ static elem get(const CliSlice& v, int i) {
    return __builtin_bit_cast(double, (static_cast<uint64_t>(v.w[2 * i + 1]) << 32) | v.w[2 * i]);
  }
};

// ---------------------------------------------------------------------------
// How a side is reached: one access of X (an element or a whole slice) at p[i].
// kShort: a slice of the side that is not whole lacks at least this many of
// its last elements (the snapshot's slices are 16-B aligned: one that the
// key's end cuts lacks its last element).
// ---------------------------------------------------------------------------
struct CliStreamed {  // the statistics' tensor, the step's g
  static constexpr int kShort = 0;
  template <typename X>
  __device__ static X ld(const X* p, int i = 0) {
    return __builtin_nontemporal_load(to_global(p) + i);
  }
};

struct CliGlobal {  // the step's w
  static constexpr int kShort = 0;
  template <typename X>
  __device__ static X ld(const X* p, int i = 0) {
    return to_global(p)[i];
  }
  template <typename X>
  __device__ static void st(X* p, X v, int i = 0) {
    to_global(p)[i] = v;
  }
};

struct CliSnapshot {
  static constexpr int kShort = 1;
  template <typename X>
  __device__ static X ld(const X* p, int i = 0) {
    return p[i];
  }
  template <typename X>
  __device__ static void st(X* p, X v, int i = 0) {
    p[i] = v;
  }
};

// elements [col, col + kPer) of a unit of n columns: one 16-B access when the
// side is 16-B aligned (VEC) and the slice is whole, else element by element
// (columns past n read as 0 and are not stored)
template <class T, class Side, bool VEC>
__device__ __forceinline__ CliSlice cli_load(const typename T::elem* p, int col, int n) {
  if (VEC && col + T::kPer <= n) return cli_slice(Side::ld(reinterpret_cast<const u32x4*>(p + col)));
  CliSlice v{{0u, 0u, 0u, 0u}};
#pragma unroll
  for (int i = 0; i < T::kPer - Side::kShort; ++i)
    if (col + i < n) T::put(v, i, Side::ld(p, col + i));
  return v;
}

template <class T, class Side, bool VEC>
__device__ __forceinline__ void cli_store(typename T::elem* p, int col, int n, const CliSlice& a) {
  if (VEC && col + T::kPer <= n) {
    Side::st(reinterpret_cast<u32x4*>(p + col), u32x4{a.w[0], a.w[1], a.w[2], a.w[3]});
  } else {
#pragma unroll
    for (int i = 0; i < T::kPer - Side::kShort; ++i)
      if (col + i < n) Side::st(p, T::get(a, i), col + i);
  }
}

// this thread's slice s starts at this column of the unit
template <class T>
__device__ __forceinline__ int cli_col(int s) {
  return T::kPer * (static_cast<int>(threadIdx.x) + s * kBlock);
}

// The workgroup's unit: its key, the unit's first column c0 in the key and
// its n columns.  A unit starts a multiple of 16 KiB into its tensor: the
// tensor's alignment is the unit's.
template <class Key>
struct CliUnit {
  Key key;
  int64_t c0;
  int n;
};

template <class T, class Key>
__device__ __forceinline__ CliUnit<Key> cli_unit(const Key* __restrict__ keys, int64_t n_keys) {
  constexpr int64_t span = kClientUnitBytes / static_cast<int64_t>(sizeof(typename T::elem));
  const int64_t u = blockIdx.x;
  const int64_t j = wave_search_last_le([&](int64_t x) { return keys[x].unit_start; }, n_keys, u);
  const Key key = keys[j];
  const int64_t c0 = (u - key.unit_start) * span;
  return {key, c0, static_cast<int>(key.numel - c0 < span ? key.numel - c0 : span)};
}

// partials[i][u]: workgroup u's NaN count (i = 0), sum x^2 (1), sum d^2 (2)
__device__ __forceinline__ void cli_store_partials(const double (&acc)[kClientStats], double* __restrict__ partials,
                                                   int64_t units) {
  __shared__ double red[kClientStats][kBlock / 64];
#pragma unroll
  for (int i = 0; i < kClientStats; ++i) {
    const double w = wave_sum_dpp(acc[i]);
    if ((threadIdx.x & 63u) == 0) red[i][threadIdx.x >> 6] = w;
  }
  __syncthreads();
  if (threadIdx.x < kClientStats) {
    double s = red[threadIdx.x][0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) s += red[threadIdx.x][w];
    partials[static_cast<int64_t>(threadIdx.x) * units + blockIdx.x] = s;
  }
}

// the body of a library's finalize kernel (one workgroup): stats[i] = sum over
// the workgroups' partials in a fixed order; stats[3] = 0
__device__ __forceinline__ void cli_finalize(const double* __restrict__ partials, int64_t units,
                                             double* __restrict__ stats) {
  __shared__ double red[kBlock];
  for (int i = 0; i < kClientStats; ++i) {
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

// ---------------------------------------------------------------------------
// The statistics pass of a rule T: T::add<HAS>(cur, snap, nans, a_cur, a_d) is
// what one slice adds; the snapshot takes the tensor's bits.
// ---------------------------------------------------------------------------
template <class T, bool HAS, bool VEC>
__device__ __forceinline__ void cli_stats_unit(const typename T::elem* __restrict__ cur,
                                               typename T::elem* __restrict__ snap, int n,
                                               double (&acc)[kClientStats]) {
  CliSlice cv[kCliC], sv[kCliC];
#pragma unroll
  for (int s = 0; s < kCliC; ++s) cv[s] = cli_load<T, CliStreamed, VEC>(cur, cli_col<T>(s), n);
#pragma unroll
  for (int s = 0; s < kCliC; ++s) {
    if constexpr (HAS)
      sv[s] = cli_load<T, CliSnapshot, true>(snap, cli_col<T>(s), n);
    else
      sv[s] = CliSlice{{0u, 0u, 0u, 0u}};
  }
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCliC; ++s) {
    T::template add<HAS>(cv[s], sv[s], nans, acc[1], acc[2]);
    cli_store<T, CliSnapshot, true>(snap, cli_col<T>(s), n, cv[s]);
  }
  acc[0] = static_cast<double>(nans);
}

template <class T, bool HAS>
__device__ __forceinline__ void cli_stats_pass(const ClientKey* __restrict__ keys, int64_t n_keys,
                                               typename T::elem* __restrict__ snap, double* __restrict__ partials,
                                               int64_t units) {
  const CliUnit<ClientKey> un = cli_unit<T>(keys, n_keys);
  const typename T::elem* cur = reinterpret_cast<const typename T::elem*>(un.key.ptr) + un.c0;
  typename T::elem* sn = snap + un.key.snap_offset + un.c0;
  double acc[kClientStats] = {0.0, 0.0, 0.0};
  if ((un.key.ptr & 15) == 0)
    cli_stats_unit<T, HAS, true>(cur, sn, un.n, acc);
  else
    cli_stats_unit<T, HAS, false>(cur, sn, un.n, acc);
  cli_store_partials(acc, partials, units);
}

// client.py:78-84's `not x or tmp > x` (:79, :83) on a running value held in a
// double; V is the type the comparison is made in
template <typename V>
__device__ __forceinline__ void track_update(double* __restrict__ x, double* __restrict__ has, V tmp) {
  const V cur = static_cast<V>(*x);
  if (*has == 0.0 || cur == static_cast<V>(0) || tmp > cur) *x = static_cast<double>(tmp);
  *has = 1.0;
}

// ---------------------------------------------------------------------------
// The scalar arithmetic of a model's type T on values held in doubles: rt(x)
// is rT(x) of an fp32 opmath result, as ATen casts it (fp32: x itself).  fp64
// models compute in fp64 and never call it.
// ---------------------------------------------------------------------------
struct CliOpF32 {
  static constexpr bool kF64 = false;
  __device__ static double rt(float x) { return static_cast<double>(x); }
};

template <class R>  // BF16Pk / F16Pk
struct CliOpHalf {
  static constexpr bool kF64 = false;
  __device__ static double rt(float x) { return static_cast<double>(R::unpack(R::pack(opaque2(f32x2{x, 0.f}))).x); }
};

struct CliOpF64 {
  static constexpr bool kF64 = true;
  __device__ static double rt(float x) { return static_cast<double>(x); }
};

// client.py:78-84 on the device in the model's type; `state` = {rho, beta,
// has rho, has beta} holds values of T exactly.  Every fp32 operation is
// formed in fp64 from fp32 operands and rounded once to fp32 (for sqrt, a
// quotient and a product of fp32 values that is the correctly rounded fp32
// result, 53 >= 2 * 24 + 2), then rounded to T as ATen casts its opmath
// result.  fp64 models: the same operations in fp64.  One thread calls it.
template <class Op>
__device__ __forceinline__ void cli_track(double* state, const double* w_stats, const double* g_stats,
                                          double abs_dloss) {
  double rho_tmp, beta_tmp;
  if constexpr (Op::kF64) {
    const double n_w = __builtin_sqrt(w_stats[2]);  // norm(w - last_w)
    const double n_g = __builtin_sqrt(g_stats[2]);  // norm(grads - last_grads)
    const double recip = 1.0 / n_w;
    rho_tmp = recip * abs_dloss;
    beta_tmp = n_g / n_w;
  } else {
    const double n_w = Op::rt(static_cast<float>(__builtin_sqrt(w_stats[2])));
    const double n_g = Op::rt(static_cast<float>(__builtin_sqrt(g_stats[2])));
    const double recip = Op::rt(static_cast<float>(1.0 / n_w));
    const double dl = static_cast<double>(static_cast<float>(abs_dloss));
    rho_tmp = Op::rt(static_cast<float>(recip * dl));
    beta_tmp = Op::rt(static_cast<float>(n_g / n_w));
  }
  track_update(state + 0, state + 2, rho_tmp);
  track_update(state + 1, state + 3, beta_tmp);
}

// ---------------------------------------------------------------------------
// The host side.  Hidden: no library exports these or binds to another's copy.
// ---------------------------------------------------------------------------
#pragma GCC visibility push(hidden)

// what a library brings to the shared host code: its error state, its own
// finalize kernel and its wording of a key whose tensor address is null or
// misaligned
struct ClientLib {
  int (*error)(int code, const char* fmt, ...);
  int (*launched)(const char* what);
  void (*finalize)(const double* partials, int64_t units, double* stats);
  int (*bad_tensor)(const char* what, int64_t key, int64_t elem_size);
};

inline int zero_stats(const ClientLib& lib, const char* what, double* stats, hipStream_t s) {
  if (!is_device_memory(stats)) return lib.error(FEDAVG_EINVAL, "%s: stats must be device memory", what);
  const hipError_t e = hipMemsetAsync(stats, 0, 4 * sizeof(double), s);
  if (e == hipSuccess) return FEDAVG_OK;
  (void)hipGetLastError();
  return lib.error(-static_cast<int>(e), "%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
}

// c: a key list's check that found no bad key
inline int check_units(const ClientLib& lib, const char* what, const ClientCheck& c, int64_t partial_elems) {
  if (c.bad == kClientTooManyUnits) return lib.error(FEDAVG_EINVAL, "%s: too many units", what);
  const int64_t need_parts = kClientStats * c.units;
  if (partial_elems < need_parts)
    return lib.error(FEDAVG_EINVAL, "%s: partials need %lld doubles", what, (long long)need_parts);
  return FEDAVG_OK;
}

inline int check_alignment(const ClientLib& lib, const char* what, const void* host_ws, const void* dev_ws,
                           const double* partials, const double* stats) {
  if (!aligned16(host_ws) || !aligned16(dev_ws) || (reinterpret_cast<uintptr_t>(partials) & 7u) ||
      (reinterpret_cast<uintptr_t>(stats) & 7u))
    return lib.error(FEDAVG_EALIGN, "%s: workspaces must be 16-B, partials and stats 8-B aligned", what);
  return FEDAVG_OK;
}

// snap: the statistics' snapshot, null for a pass without one
inline int check_memory(const ClientLib& lib, const char* what, const void* host_ws, const void* dev_ws,
                        const void* snap, const double* partials, const double* stats) {
  if (!is_pinned_host_memory(host_ws)) return lib.error(FEDAVG_EINVAL, "%s: host_ws is not pinned host memory", what);
  if (!is_device_memory(dev_ws) || (snap && !is_device_memory(snap)) || !is_device_memory(partials) ||
      !is_device_memory(stats))
    return lib.error(FEDAVG_EINVAL, snap ? "%s: dev_ws, snap, partials and stats must be device memory"
                                         : "%s: dev_ws, partials and stats must be device memory",
                     what);
  return FEDAVG_OK;
}

// a host address would fault the kernel: spot check of the first and last
// tensor of a side (the Python layer checks every tensor's device)
inline int check_tensors(const ClientLib& lib, const char* what, const int64_t* side, const ClientFill& f) {
  if (!is_device_memory(reinterpret_cast<const void*>(side[f.first])) ||
      !is_device_memory(reinterpret_cast<const void*>(side[f.last])))
    return lib.error(FEDAVG_EINVAL, "%s: the tensors must be device memory", what);
  return FEDAVG_OK;
}

// the one H2D of the staged table, pass(), then fin(): the launch that adds the partials up
template <class Pass, class Fin>
int stage_then(const ClientLib& lib, const char* what, const void* host_ws, void* dev_ws, int64_t ws_bytes,
               hipStream_t s, Pass pass, Fin fin) {
  const hipError_t e = hipMemcpyAsync(dev_ws, host_ws, static_cast<size_t>(ws_bytes), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return lib.error(-static_cast<int>(e), "%s: hipMemcpyAsync failed: %s", what, hipGetErrorString(e));
  }
  pass();
  const int rc = lib.launched(what);
  if (rc) return rc;
  fin();
  return lib.launched(what);
}

// the same with the library's own finalize
template <class Pass>
int stage_and_launch(const ClientLib& lib, const char* what, const void* host_ws, void* dev_ws, int64_t ws_bytes,
                     double* partials, int64_t units, double* stats, hipStream_t s, Pass pass) {
  return stage_then(lib, what, host_ws, dev_ws, ws_bytes, s, pass, [&] {
    hipLaunchKernelGGL(lib.finalize, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  });
}

// A statistics entry point of rule T; kernels[has_snap] is the library's pass.
template <class T>
int client_stats_entry(const ClientLib& lib, const char* what,
                       void (*const (&kernels)[2])(const ClientKey*, int64_t, typename T::elem*, double*, int64_t),
                       const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys,
                       typename T::elem* snap, int64_t P, int has_snap, double* partials, int64_t partial_elems,
                       double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0 || P < 0) return lib.error(FEDAVG_EINVAL, "%s: negative n_keys or P", what);
  if (!stats) return lib.error(FEDAVG_EINVAL, "%s: null stats", what);
  if (P == 0 || n_keys == 0) return zero_stats(lib, what, stats, s);
  if (!cur_ptrs || !key_numel || !key_offset || !snap || !partials || !host_ws || !dev_ws)
    return lib.error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = client_workspace(n_keys);
  if (ws_bytes < need_ws) return lib.error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  const ClientCheck keys_ok = client_check_stats_keys(cur_ptrs, key_numel, key_offset, n_keys, P, es);
  if (keys_ok.bad == kClientOutside)
    return lib.error(FEDAVG_EINVAL, "%s: key %lld lies outside the snapshot of %lld elements", what,
                     (long long)keys_ok.key, (long long)P);
  if (keys_ok.bad == kClientBadTensor)
    return lib.bad_tensor(what, keys_ok.key, es);
  if (const int rc = check_units(lib, what, keys_ok, partial_elems)) return rc;
  const int64_t units = keys_ok.units;
  if (!aligned16(snap)) return lib.error(FEDAVG_EALIGN, "%s: snap must be 16-B aligned", what);
  const ClientCheck offsets_ok = client_check_snap_offsets(key_offset, n_keys, es);
  if (offsets_ok.bad)
    return lib.error(FEDAVG_EALIGN, "%s: key %lld: snapshot offset must be a multiple of %lld elements", what,
                     (long long)offsets_ok.key, (long long)(16 / es));
  if (const int rc = check_alignment(lib, what, host_ws, dev_ws, partials, stats)) return rc;
  if (units == 0) return zero_stats(lib, what, stats, s);
  if (const int rc = check_memory(lib, what, host_ws, dev_ws, snap, partials, stats)) return rc;
  const ClientFill f = client_fill(static_cast<ClientKey*>(host_ws), key_numel, n_keys, client_span(es),
                                   [&](int64_t j, int64_t unit_start) {
                                     return ClientKey{cur_ptrs[j], key_numel[j], key_offset[j], unit_start};
                                   });
  if (const int rc = check_tensors(lib, what, cur_ptrs, f)) return rc;
  return stage_and_launch(lib, what, host_ws, dev_ws, need_ws, partials, units, stats, s, [&] {
    hipLaunchKernelGGL(kernels[has_snap ? 1 : 0], dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s,
                       static_cast<const ClientKey*>(dev_ws), n_keys, snap, partials, units);
  });
}

// a track entry point: three records of doubles on the device, one thread of `kernel`
inline int client_track_entry(const ClientLib& lib, const char* what,
                              void (*kernel)(double*, const double*, const double*, double), double* state,
                              const double* w_stats, const double* g_stats, double abs_dloss, void* stream) {
  if (!state || !w_stats || !g_stats) return lib.error(FEDAVG_EINVAL, "%s: null argument", what);
  if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(w_stats) |
       reinterpret_cast<uintptr_t>(g_stats)) & 7u)
    return lib.error(FEDAVG_EALIGN, "%s: records must be 8-B aligned", what);
  if (!is_device_memory(state) || !is_device_memory(w_stats) || !is_device_memory(g_stats))
    return lib.error(FEDAVG_EINVAL, "%s: state and records must be device memory", what);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, w_stats, g_stats,
                     abs_dloss);
  return lib.launched(what);
}

#pragma GCC visibility pop

}  // namespace fedavg_impl
