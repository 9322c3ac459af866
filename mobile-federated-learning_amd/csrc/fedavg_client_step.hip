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
// The pass is client_pass.hpp's, with w and g as the key's two sides; this
// file holds the step of each dtype, the kernels' entry points and the C ABI.
#include "client_pass.hpp"

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

__device__ __forceinline__ void add_sq(double& acc, double x) { acc = __builtin_fma(x, x, acc); }

// ---------------------------------------------------------------------------
// Dtype rules: the opmath type and the step of one slice: out = w', {NaN
// count, sum w'^2, sum d^2} += its first `live` elements (the others are
// columns past the key's end: whatever alpha makes of their zeros counts as
// nothing).
// ---------------------------------------------------------------------------
struct CsF32 : CliElem<4> {
  typedef float op;
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

template <class T, int FORM>
__global__ __launch_bounds__(kBlock) void client_sgd_step_kernel(const StepKey* __restrict__ keys, int64_t n_keys,
                                                                 typename T::op alpha, double* __restrict__ partials,
                                                                 int64_t units) {
  const CliUnit<StepKey> un = cli_unit<T>(keys, n_keys);
  typename T::elem* w = reinterpret_cast<typename T::elem*>(un.key.w) + un.c0;
  const typename T::elem* g = reinterpret_cast<const typename T::elem*>(un.key.g) + un.c0;
  double acc[kClientStats] = {0.0, 0.0, 0.0};
  const bool wvec = (un.key.w & 15) == 0, gvec = (un.key.g & 15) == 0;
  if (wvec && gvec)
    step_unit<T, FORM, true, true>(w, g, un.n, alpha, acc);
  else if (wvec)
    step_unit<T, FORM, true, false>(w, g, un.n, alpha, acc);
  else if (gvec)
    step_unit<T, FORM, false, true>(w, g, un.n, alpha, acc);
  else
    step_unit<T, FORM, false, false>(w, g, un.n, alpha, acc);
  cli_store_partials(acc, partials, units);
}

__global__ __launch_bounds__(kBlock) void client_sgd_step_finalize_kernel(const double* __restrict__ partials,
                                                                          int64_t units, double* __restrict__ stats) {
  cli_finalize(partials, units, stats);
}

int bad_tensor(const char* what, int64_t key, int64_t elem_size) {
  return cs_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                  (long long)key, (long long)elem_size);
}

const ClientLib kLib = {cs_error, cs_launch_status, client_sgd_step_finalize_kernel, bad_tensor};

template <class T>
int client_sgd_step(const char* what, const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                    int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems, double* stats,
                    void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  constexpr int64_t es = static_cast<int64_t>(sizeof(typename T::elem));
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (n_keys < 0) return cs_error(FEDAVG_EINVAL, "%s: negative n_keys", what);
  if (!stats) return cs_error(FEDAVG_EINVAL, "%s: null stats", what);
  if (form != 0 && form != 1) return cs_error(FEDAVG_EMODE, "%s: form %d is neither 0 nor 1", what, form);
  if (n_keys == 0) return zero_stats(kLib, what, stats, s);
  if (!w_ptrs || !g_ptrs || !key_numel || !partials || !host_ws || !dev_ws)
    return cs_error(FEDAVG_EINVAL, "%s: null argument", what);
  const int64_t need_ws = client_workspace(n_keys);
  if (ws_bytes < need_ws) return cs_error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)need_ws);
  const ClientCheck keys_ok = client_check_step_keys(w_ptrs, g_ptrs, key_numel, n_keys, es);
  if (keys_ok.bad == kClientNegative)
    return cs_error(FEDAVG_EINVAL, "%s: key %lld: negative size", what, (long long)keys_ok.key);
  if (keys_ok.bad == kClientBadTensor)
    return bad_tensor(what, keys_ok.key, es);
  if (const int rc = check_units(kLib, what, keys_ok, partial_elems)) return rc;
  const int64_t units = keys_ok.units;
  if (const int rc = check_alignment(kLib, what, host_ws, dev_ws, partials, stats)) return rc;
  if (units == 0) return zero_stats(kLib, what, stats, s);
  if (const int rc = check_memory(kLib, what, host_ws, dev_ws, nullptr, partials, stats)) return rc;
  const ClientFill f = client_fill(static_cast<StepKey*>(host_ws), key_numel, n_keys, client_span(es),
                                   [&](int64_t j, int64_t unit_start) {
                                     return StepKey{w_ptrs[j], g_ptrs[j], key_numel[j], unit_start};
                                   });
  for (const int64_t* side : {w_ptrs, g_ptrs})
    if (const int rc = check_tensors(kLib, what, side, f)) return rc;
  const typename T::op alpha = static_cast<typename T::op>(-lr);  // ATen: the scalar rounded once to opmath
  return stage_and_launch(kLib, what, host_ws, dev_ws, need_ws, partials, units, stats, s, [&] {
    hipLaunchKernelGGL((form ? client_sgd_step_kernel<T, 1> : client_sgd_step_kernel<T, 0>),
                       dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, static_cast<const StepKey*>(dev_ws),
                       n_keys, alpha, partials, units);
  });
}

}  // namespace

extern "C" {

int fedavg_clientstep_abi_version(void) { return 1; }

const char* fedavg_clientstep_last_error(void) { return g_cs_err.c_str(); }

int64_t fedavg_client_step_span(int64_t elem_size) { return client_span(elem_size); }

int64_t fedavg_client_step_workspace(int64_t n_keys) { return client_workspace(n_keys); }

int64_t fedavg_client_step_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  return client_partials(key_numel, n_keys, client_span(elem_size));
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
