// client_adam_rules.hpp -- the client's Adam step (client.py:43-44,
// torch.optim.Adam with coupled weight decay and amsgrad) fused with the
// weight statistics of :76-82, once: the arithmetic of one element, the step
// of each dtype, one unit, the body of the step kernel and the checks and
// staging of an entry point.  fedavg_client_adam.hip
// (libfedavg_amd_clientadam.so) and fedavg_client_loop.hip
// (libfedavg_amd_clientloop.so, the same step behind a gate) include it and
// add their __global__ entry points and their C ABI.
//
// The rules live in an anonymous namespace: each library's kernels carry them
// in their names as its own types, and no library exports them.
#pragma once

#include "client_pass.hpp"

#include "client_adam_plan.hpp"

namespace {
using namespace fedavg_impl;

// the coefficients in opmath, the form mask and whether op A exists
template <class S>
struct AdamCoef {
  S wd, lw, beta2, value, bc2s, eps, step;
  int form, has_wd;
};

// ---------------------------------------------------------------------------
// The arithmetic on a value V (float, double, or two floats of a packed 16-bit
// word) with scalars S; Rnd::r rounds an opmath value to the model's type.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ f32x2 fma_(float a, f32x2 b, f32x2 c) {
  return f32x2{__builtin_fmaf(a, b.x, c.x), __builtin_fmaf(a, b.y, c.y)};
}
__device__ __forceinline__ float sqrt_(float a) { return __builtin_sqrtf(a); }
__device__ __forceinline__ double sqrt_(double a) { return __builtin_sqrt(a); }
__device__ __forceinline__ f32x2 sqrt_(f32x2 a) { return f32x2{__builtin_sqrtf(a.x), __builtin_sqrtf(a.y)}; }
// ATen's maximum functor: (isnan(a) || a > b) ? a : b
__device__ __forceinline__ float max_nan(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ double max_nan(double a, double b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ f32x2 max_nan(f32x2 a, f32x2 b) { return f32x2{max_nan(a.x, b.x), max_nan(a.y, b.y)}; }

struct RndNone {
  template <class V>
  __device__ static V r(V x) {
    return x;
  }
};

template <class R>  // BF16Pk / F16Pk: to the type and back, never one mixed-precision operation
struct RndHalf {
  __device__ static f32x2 r(f32x2 x) { return R::unpack(R::pack(opaque2(x))); }
};

template <class V>
struct AdamOut {
  V w, m, v, x, d;
};

template <class Rnd, class V, class S>
__device__ __forceinline__ AdamOut<V> adam_elem(V w, V g, V m, V v, V x, const AdamCoef<S> c) {
  V g1 = g;
  if (c.has_wd) g1 = Rnd::r((c.form & 1) ? fma_(c.wd, w, g) : g + c.wd * w);
  const V diff = g1 - m;
  const V mn = Rnd::r((c.form & 2) ? fma_(c.lw, diff, m) : m + c.lw * diff);
  const V v1 = Rnd::r(v * c.beta2);
  const V gg = g1 * g1;
  const V vn = Rnd::r((c.form & 4) ? fma_(c.value, gg, v1) : v1 + c.value * gg);
  const V xn = max_nan(x, vn);
  const V s1 = Rnd::r(sqrt_(xn));
  const V s2 = Rnd::r(s1 / c.bc2s);
  const V s3 = Rnd::r(s2 + c.eps);
  const V q = mn / s3;
  const V wn = Rnd::r((c.form & 8) ? fma_(c.step, q, w) : w + c.step * q);
  return {wn, mn, vn, xn, Rnd::r(wn - w)};
}

// the five slices of one 16 B of a key: w, g and the state planes
struct AdamSlices {
  CliSlice w, g, m, v, x;
};

// ---------------------------------------------------------------------------
// Dtype rules: the opmath type, the slices a thread keeps in flight, and the
// step of one slice: s.w / s.m / s.v / s.x become w', m', v', vmax' and {NaN
// count, sum w'^2, sum d^2} += its first `live` elements.
// ---------------------------------------------------------------------------
struct CaF32 : CliElem<4> {
  typedef float op;
  typedef CliOpF32 scalar;
  static constexpr int kFlight = 4;
  __device__ __forceinline__ static void step(AdamSlices& s, const AdamCoef<op> c, int live, int& nans, double& a_w,
                                              double& a_d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const AdamOut<float> o =
          adam_elem<RndNone>(__uint_as_float(s.w.w[k]), __uint_as_float(s.g.w[k]), __uint_as_float(s.m.w[k]),
                             __uint_as_float(s.v.w[k]), __uint_as_float(s.x.w[k]), c);
      s.w.w[k] = __float_as_uint(o.w);
      s.m.w[k] = __float_as_uint(o.m);
      s.v.w[k] = __float_as_uint(o.v);
      s.x.w[k] = __float_as_uint(o.x);
      const bool on = k < live;
      nans += static_cast<int>(on && o.w != o.w);
      add_sq(a_w, on ? static_cast<double>(o.w) : 0.0);  // the fp64 square of an fp32 value is exact
      add_sq(a_d, on ? static_cast<double>(o.d) : 0.0);
    }
  }
};

// bf16 / fp16; R = BF16Pk / F16Pk (common.hpp): two elements per 32-bit word
template <class R>
struct CaHalf : CliElem<2> {
  typedef float op;
  typedef CliOpHalf<R> scalar;
  static constexpr int kFlight = 2;
  __device__ __forceinline__ static void step(AdamSlices& s, const AdamCoef<op> c, int live, int& nans, double& a_w,
                                              double& a_d) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const AdamOut<f32x2> o = adam_elem<RndHalf<R>>(R::unpack(s.w.w[k]), R::unpack(s.g.w[k]), R::unpack(s.m.w[k]),
                                                     R::unpack(s.v.w[k]), R::unpack(s.x.w[k]), c);
      s.w.w[k] = R::pack(o.w);  // already values of the type: exact
      s.m.w[k] = R::pack(o.m);
      s.v.w[k] = R::pack(o.v);
      s.x.w[k] = R::pack(o.x);
      const bool on0 = 2 * k < live, on1 = 2 * k + 1 < live;
      nans += static_cast<int>(on0 && o.w.x != o.w.x) + static_cast<int>(on1 && o.w.y != o.w.y);
      add_sq(a_w, on0 ? static_cast<double>(o.w.x) : 0.0);  // the fp64 square of a widened 16-bit value is exact
      add_sq(a_w, on1 ? static_cast<double>(o.w.y) : 0.0);
      add_sq(a_d, on0 ? static_cast<double>(o.d.x) : 0.0);
      add_sq(a_d, on1 ? static_cast<double>(o.d.y) : 0.0);
    }
  }
};

struct CaF64 : CliElem<8> {
  typedef double op;
  typedef CliOpF64 scalar;
  static constexpr int kFlight = 2;
  __device__ __forceinline__ static void step(AdamSlices& s, const AdamCoef<op> c, int live, int& nans, double& a_w,
                                              double& a_d) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const AdamOut<double> o = adam_elem<RndNone>(get(s.w, k), get(s.g, k), get(s.m, k), get(s.v, k), get(s.x, k), c);
      put(s.w, k, o.w);
      put(s.m, k, o.m);
      put(s.v, k, o.v);
      put(s.x, k, o.x);
      const bool on = k < live;
      nans += static_cast<int>(on && o.w != o.w);
      add_sq(a_w, on ? o.w : 0.0);
      add_sq(a_d, on ? o.d : 0.0);
    }
  }
};

// the state: global, plain, always 16-B aligned; a slice the key's end cuts lacks its last element
struct CliState {
  static constexpr int kShort = 1;
  template <typename X>
  __device__ static X ld(const X* p, int i = 0) {
    return to_global(p)[i];
  }
  template <typename X>
  __device__ static void st(X* p, X v, int i = 0) {
    to_global(p)[i] = v;
  }
};

// elements [col, col + kPer) of a side whose 16-B alignment `vec` is uniform over the workgroup: client_pass.hpp's
// two paths behind one branch, so that the arithmetic below them exists once per kernel
template <class T, class Side>
__device__ __forceinline__ CliSlice adam_load(const typename T::elem* p, int col, int n, bool vec) {
  if (vec && col + T::kPer <= n) return cli_load<T, Side, true>(p, col, n);
  return cli_load<T, Side, false>(p, col, n);
}

template <class T, class Side>
__device__ __forceinline__ void adam_store(typename T::elem* p, int col, int n, bool vec, const CliSlice& a) {
  if (vec && col + T::kPer <= n)
    cli_store<T, Side, true>(p, col, n, a);
  else
    cli_store<T, Side, false>(p, col, n, a);
}

// One unit: this thread's kCliC slices, T::kFlight of them in flight at a
// time; acc = {NaN count, sum w'^2, sum d^2}.  st: the key's place in plane 0.
template <class T, bool FIRST>
__device__ __forceinline__ void adam_unit(typename T::elem* w, const typename T::elem* g, typename T::elem* st,
                                          int64_t plane, int n, bool wvec, bool gvec,
                                          const AdamCoef<typename T::op> c, double (&acc)[kClientStats]) {
  constexpr int F = T::kFlight;
  static_assert(kCliC % F == 0, "whole batches");
  typename T::elem* const m = st;
  typename T::elem* const v = st + plane;
  typename T::elem* const x = st + 2 * plane;
  int nans = 0;
#pragma unroll
  for (int b = 0; b < kCliC; b += F) {
    AdamSlices sl[F];
#pragma unroll
    for (int s = 0; s < F; ++s) sl[s].w = adam_load<T, CliGlobal>(w, cli_col<T>(b + s), n, wvec);
#pragma unroll
    for (int s = 0; s < F; ++s) sl[s].g = adam_load<T, CliStreamed>(g, cli_col<T>(b + s), n, gvec);
#pragma unroll
    for (int s = 0; s < F; ++s) {
      if constexpr (FIRST) {
        sl[s].m = sl[s].v = sl[s].x = CliSlice{{0u, 0u, 0u, 0u}};  // +0 in every type
      } else {
        sl[s].m = cli_load<T, CliState, true>(m, cli_col<T>(b + s), n);
        sl[s].v = cli_load<T, CliState, true>(v, cli_col<T>(b + s), n);
        sl[s].x = cli_load<T, CliState, true>(x, cli_col<T>(b + s), n);
      }
    }
#pragma unroll
    for (int s = 0; s < F; ++s) {
      const int col = cli_col<T>(b + s);
      T::step(sl[s], c, n - col, nans, acc[1], acc[2]);
      adam_store<T, CliGlobal>(w, col, n, wvec, sl[s].w);
      cli_store<T, CliState, true>(m, col, n, sl[s].m);
      cli_store<T, CliState, true>(v, col, n, sl[s].v);
      cli_store<T, CliState, true>(x, col, n, sl[s].x);
    }
  }
  acc[0] = static_cast<double>(nans);
}

// the body of a step kernel: this workgroup's unit and its three partials
template <class T, bool FIRST>
__device__ __forceinline__ void adam_step_pass(const AdamKey* __restrict__ keys, int64_t n_keys,
                                               typename T::elem* __restrict__ state, int64_t plane,
                                               const AdamCoef<typename T::op> c, double* __restrict__ partials,
                                               int64_t units) {
  const CliUnit<AdamKey> un = cli_unit<T>(keys, n_keys);
  typename T::elem* w = reinterpret_cast<typename T::elem*>(un.key.w) + un.c0;
  const typename T::elem* g = reinterpret_cast<const typename T::elem*>(un.key.g) + un.c0;
  typename T::elem* st = state + un.key.state_offset + un.c0;
  double acc[kClientStats] = {0.0, 0.0, 0.0};
  adam_unit<T, FIRST>(w, g, st, plane, un.n, (un.key.w & 15) == 0, (un.key.g & 15) == 0, c, acc);
  cli_store_partials(acc, partials, units);
}

// ---------------------------------------------------------------------------
// The host side of a step entry point of rule T: every check, the staged table
// and the two launches.  What differs between a library's entries is its
// Launch:
//   int  empty(what, stats, s)      nothing to step: the record of no elements
//   int  memory(what)               the memory checks of what the library adds
//   void step<T>(first, keys, n_keys, state, state_elems, coef, partials, units, s)
//   void finalize(partials, units, stats, s)
// ---------------------------------------------------------------------------
template <class T, class Launch>
int adam_step_entry(const ClientLib& lib, const Launch& launch, const char* what, const int64_t* w_ptrs,
                    const int64_t* g_ptrs, const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys,
                    void* state, int64_t state_elems, const double* coef, int first, int form, double* partials,
                    int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                    void* stream) {
  typedef typename T::op op;
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0 || state_elems < 0) return lib.error(FEDAVG_EINVAL, "%s: negative n_keys or state_elems", what);
  if (!stats) return lib.error(FEDAVG_EINVAL, "%s: null stats", what);
  if (!coef) return lib.error(FEDAVG_EINVAL, "%s: null coef", what);
  if (!adam_form_ok(form)) return lib.error(FEDAVG_EMODE, "%s: form %d is no mask of the 4 sites (0..15)", what, form);
  if (!adam_lerp_weight_ok(coef[1]))
    return lib.error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                     coef[1]);
  if (n_keys == 0) return launch.empty(what, stats, s);
  if (!w_ptrs || !g_ptrs || !key_numel || !key_offset || !state || !partials || !host_ws || !dev_ws)
    return lib.error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = adam_workspace(n_keys);
  if (ws_bytes < need_ws) return lib.error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  const ClientCheck keys_ok = adam_check_keys(w_ptrs, g_ptrs, key_numel, key_offset, n_keys, state_elems, es);
  if (keys_ok.bad == kClientNegative)
    return lib.error(FEDAVG_EINVAL, "%s: key %lld: negative size", what, (long long)keys_ok.key);
  if (keys_ok.bad == kClientBadTensor) return lib.bad_tensor(what, keys_ok.key, es);
  if (keys_ok.bad == kClientOutside)
    return lib.error(FEDAVG_EINVAL, "%s: key %lld lies outside a state plane of %lld elements", what,
                     (long long)keys_ok.key, (long long)state_elems);
  if (keys_ok.bad == kClientBadOffset)
    return lib.error(FEDAVG_EALIGN, "%s: key %lld: state offset must be a multiple of %lld elements", what,
                     (long long)keys_ok.key, (long long)(16 / es));
  if (const int rc = check_units(lib, what, keys_ok, partial_elems)) return rc;
  const int64_t units = keys_ok.units;
  if (!aligned16(state) || state_elems % (16 / es))
    return lib.error(FEDAVG_EALIGN, "%s: state must be 16-B aligned and state_elems a multiple of %lld elements", what,
                     (long long)(16 / es));
  if (const int rc = check_alignment(lib, what, host_ws, dev_ws, partials, stats)) return rc;
  if (units == 0) return launch.empty(what, stats, s);
  if (!is_device_memory(state)) return lib.error(FEDAVG_EINVAL, "%s: state must be device memory", what);
  if (const int rc = check_memory(lib, what, host_ws, dev_ws, nullptr, partials, stats)) return rc;
  if (const int rc = launch.memory(what)) return rc;
  const ClientFill f = client_fill(static_cast<AdamKey*>(host_ws), key_numel, n_keys, client_span(es),
                                   [&](int64_t j, int64_t unit_start) {
                                     return AdamKey{w_ptrs[j], g_ptrs[j], key_numel[j], key_offset[j], unit_start};
                                   });
  for (const int64_t* side : {w_ptrs, g_ptrs})
    if (const int rc = check_tensors(lib, what, side, f)) return rc;
  // ATen: every scalar rounded once to opmath
  const AdamCoef<op> c = {static_cast<op>(coef[0]), static_cast<op>(coef[1]), static_cast<op>(coef[2]),
                          static_cast<op>(coef[3]), static_cast<op>(coef[4]), static_cast<op>(coef[5]),
                          static_cast<op>(coef[6]), form,                     coef[0] != 0.0 ? 1 : 0};
  return stage_then(
      lib, what, host_ws, dev_ws, need_ws, s,
      [&] {
        launch.template step<T>(first != 0, static_cast<const AdamKey*>(dev_ws), n_keys,
                                static_cast<typename T::elem*>(state), state_elems, c, partials, units, s);
      },
      [&] { launch.finalize(partials, units, stats, s); });
}

}  // namespace
