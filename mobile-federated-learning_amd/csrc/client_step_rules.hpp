// client_step_rules.hpp -- the client's plain SGD step (client.py:74) fused
// with the weight statistics of :76-82, once: the step of each dtype, one
// unit and the checks and staging of an entry point.  fedavg_client_step.hip (libfedavg_amd_clientstep.so) and
// fedavg_client_loop.hip (libfedavg_amd_clientloop.so, the same step behind a
// gate) include it and add their __global__ entry points and their C ABI.
//
// The rules live in an anonymous namespace: each library's kernels carry them
// in their names as its own types, and no library exports them.
#pragma once

#include "client_pass.hpp"

namespace {
using namespace fedavg_impl;

// ---------------------------------------------------------------------------
// Dtype rules: the opmath type and the step of one slice: out = w', {NaN
// count, sum w'^2, sum d^2} += its first `live` elements (the others are
// columns past the key's end: whatever alpha makes of their zeros counts as
// nothing).
// ---------------------------------------------------------------------------
struct CsF32 : CliElem<4> {
  typedef float op;
  typedef CliOpF32 scalar;
  template <int FORM>
  __device__ static void step(const CliSlice& c, const CliSlice& g, op alpha, int live, CliSlice& out, int& nans,
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
struct CsHalf : CliElem<2> {
  typedef float op;
  typedef CliOpHalf<R> scalar;
  template <int FORM>
  __device__ static void step(const CliSlice& c, const CliSlice& g, op alpha, int live, CliSlice& out, int& nans,
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

struct CsF64 : CliElem<8> {
  typedef double op;
  typedef CliOpF64 scalar;
  template <int FORM>
  __device__ static void step(const CliSlice& c, const CliSlice& g, op alpha, int live, CliSlice& out, int& nans,
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

// one unit: this thread's kCliC slices; acc = {NaN count, sum w'^2, sum d^2}
template <class T, int FORM, bool WVEC, bool GVEC>
__device__ __forceinline__ void step_unit(typename T::elem* w, const typename T::elem* g, int n, typename T::op alpha,
                                          double (&acc)[kClientStats]) {
  CliSlice wv[kCliC], gv[kCliC];
#pragma unroll
  for (int s = 0; s < kCliC; ++s) wv[s] = cli_load<T, CliGlobal, WVEC>(w, cli_col<T>(s), n);
#pragma unroll
  for (int s = 0; s < kCliC; ++s) gv[s] = cli_load<T, CliStreamed, GVEC>(g, cli_col<T>(s), n);
  int nans = 0;
#pragma unroll
  for (int s = 0; s < kCliC; ++s) {
    const int col = cli_col<T>(s);
    CliSlice out;
    T::template step<FORM>(wv[s], gv[s], alpha, n - col, out, nans, acc[1], acc[2]);
    cli_store<T, CliGlobal, WVEC>(w, col, n, out);
  }
  acc[0] = static_cast<double>(nans);
}

// ---------------------------------------------------------------------------
// The host side of a step entry point of rule T: every check, the staged table
// and the two launches.  What differs between a library's entries is its
// Launch:
//   int  empty(what, stats, s)      nothing to step: the record of no elements
//   int  memory(what)               the memory checks of what the library adds
//   void step<T>(form, keys, n_keys, alpha, partials, units, s)
//   void finalize(partials, units, stats, s)
// ---------------------------------------------------------------------------
template <class T, class Launch>
int sgd_step_entry(const ClientLib& lib, const Launch& launch, const char* what, const int64_t* w_ptrs,
                   const int64_t* g_ptrs, const int64_t* key_numel, int64_t n_keys, double lr, int form,
                   double* partials, int64_t partial_elems, double* stats, void* host_ws, void* dev_ws,
                   int64_t ws_bytes, void* stream) {
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0) return lib.error(FEDAVG_EINVAL, "%s: negative n_keys", what);
  if (!stats) return lib.error(FEDAVG_EINVAL, "%s: null stats", what);
  if (form != 0 && form != 1) return lib.error(FEDAVG_EMODE, "%s: form %d is neither 0 nor 1", what, form);
  if (n_keys == 0) return launch.empty(what, stats, s);
  if (!w_ptrs || !g_ptrs || !key_numel || !partials || !host_ws || !dev_ws)
    return lib.error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = client_workspace(n_keys);
  if (ws_bytes < need_ws) return lib.error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  const ClientCheck keys_ok = client_check_step_keys(w_ptrs, g_ptrs, key_numel, n_keys, es);
  if (keys_ok.bad == kClientNegative)
    return lib.error(FEDAVG_EINVAL, "%s: key %lld: negative size", what, (long long)keys_ok.key);
  if (keys_ok.bad == kClientBadTensor) return lib.bad_tensor(what, keys_ok.key, es);
  if (const int rc = check_units(lib, what, keys_ok, partial_elems)) return rc;
  const int64_t units = keys_ok.units;
  if (const int rc = check_alignment(lib, what, host_ws, dev_ws, partials, stats)) return rc;
  if (units == 0) return launch.empty(what, stats, s);
  if (const int rc = check_memory(lib, what, host_ws, dev_ws, nullptr, partials, stats)) return rc;
  if (const int rc = launch.memory(what)) return rc;
  const ClientFill f = client_fill(static_cast<StepKey*>(host_ws), key_numel, n_keys, client_span(es),
                                   [&](int64_t j, int64_t unit_start) {
                                     return StepKey{w_ptrs[j], g_ptrs[j], key_numel[j], unit_start};
                                   });
  for (const int64_t* side : {w_ptrs, g_ptrs})
    if (const int rc = check_tensors(lib, what, side, f)) return rc;
  const typename T::op alpha = static_cast<typename T::op>(-lr);  // ATen: the scalar rounded once to opmath
  return stage_then(
      lib, what, host_ws, dev_ws, need_ws, s,
      [&] {
        launch.template step<T>(form, static_cast<const StepKey*>(dev_ws), n_keys, alpha, partials, units, s);
      },
      [&] { launch.finalize(partials, units, stats, s); });
}

}  // namespace
