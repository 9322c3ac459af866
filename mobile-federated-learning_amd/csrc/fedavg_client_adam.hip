// fedavg_client_adam.hip -- libfedavg_amd_clientadam.so (include/
// fedavg_amd_clientadam.h): the client's Adam step (client.py:43-44,
// torch.optim.Adam with coupled weight decay and amsgrad) and the weight
// statistics of :76-82 in one pass, for fp32, bf16, fp16 and fp64 models.
//
// torch's multi-tensor Adam is nine elementwise launches per step, each of
// which stores its result in the model's type T.  Here one kernel reads w, g
// and the three state planes m, v, vmax and forms, every line rounded to T
// (rT) as the foreach op behind it stores it:
//     A  g1    = rT(g + wd * w)               no op at all when wd == 0
//     B  m'    = rT(m + lw * (g1 - m))        Lerp.h, |lw| < 0.5
//        v1    = rT(v * beta2)
//     C  v'    = rT(v1 + value * (g1 * g1))
//        vmax' = max(vmax, v')                a NaN on either side stays
//        s1    = rT(sqrt(vmax'))
//        s2    = rT(s1 / bc2s)
//        s3    = rT(s2 + eps)
//     E  w'    = rT(w + step * (m' / s3))
//        d     = rT(w' - w)                   the difference in the model's type (:78)
//        count of isnan(w'), sum w'^2, sum d^2        (squares and sums in fp64)
// and stores w', m', v', vmax': 36 B per fp32 element, no weight snapshot.  A
// first step (all state +0) does not read the state: 24 B.  A, B, C and E are
// x + s * y; bit i of `form` makes site i one __builtin_fma[f], a clear bit
// leaves product and sum rounded apart (the unit is -ffp-contract=off and
// common.hpp pins it).  `form` is a kernel argument, uniform over the launch:
// one instance per dtype and first / later step.  Which mask equals torch's
// bits is the caller's finding (client_stats.adam_form).
//
// The pass is client_pass.hpp's, with w and g as the key's two sides and the
// state as a third, always 16-B aligned one; the arithmetic, the kernel's body
// and an entry point's checks are client_adam_rules.hpp's (shared with the
// gated step of fedavg_client_loop.hip); this file holds the kernels' entry
// points and the C ABI.
#include "client_adam_rules.hpp"

#include "fedavg_amd_clientadam.h"

namespace {

thread_local ErrorState g_ca_err;

int ca_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_ca_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int ca_launch_status(const char* what) { return launch_status(g_ca_err, what); }

template <class T, bool FIRST>
__global__ __launch_bounds__(kBlock) void client_adam_step_kernel(const AdamKey* __restrict__ keys, int64_t n_keys,
                                                                  typename T::elem* __restrict__ state, int64_t plane,
                                                                  typename T::op wd, typename T::op lw,
                                                                  typename T::op beta2, typename T::op value,
                                                                  typename T::op bc2s, typename T::op eps,
                                                                  typename T::op step, int form, int has_wd,
                                                                  double* __restrict__ partials, int64_t units) {
  const AdamCoef<typename T::op> c = {wd, lw, beta2, value, bc2s, eps, step, form, has_wd};
  adam_step_pass<T, FIRST>(keys, n_keys, state, plane, c, partials, units);
}

__global__ __launch_bounds__(kBlock) void client_adam_step_finalize_kernel(const double* __restrict__ partials,
                                                                           int64_t units, double* __restrict__ stats) {
  cli_finalize(partials, units, stats);
}

int bad_tensor(const char* what, int64_t key, int64_t elem_size) {
  return ca_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                  (long long)key, (long long)elem_size);
}

const ClientLib kLib = {ca_error, ca_launch_status, client_adam_step_finalize_kernel, bad_tensor};

// this library's launches: the step as it is, stats = 0 by a memset where there is nothing to step
struct PlainStep {
  int empty(const char* what, double* stats, hipStream_t s) const { return zero_stats(kLib, what, stats, s); }
  int memory(const char*) const { return FEDAVG_OK; }
  template <class T>
  void step(bool first, const AdamKey* keys, int64_t n_keys, typename T::elem* state, int64_t state_elems,
            const AdamCoef<typename T::op>& c, double* partials, int64_t units, hipStream_t s) const {
    hipLaunchKernelGGL((first ? client_adam_step_kernel<T, true> : client_adam_step_kernel<T, false>),
                       dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys, n_keys, state, state_elems, c.wd,
                       c.lw, c.beta2, c.value, c.bc2s, c.eps, c.step, c.form, c.has_wd, partials, units);
  }
  void finalize(const double* partials, int64_t units, double* stats, hipStream_t s) const {
    hipLaunchKernelGGL(client_adam_step_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  }
};

template <class T, class... Args>
int client_adam_step(const char* what, Args... args) {
  return adam_step_entry<T>(kLib, PlainStep{}, what, args...);
}

}  // namespace

#define FEDAVG_ADAM_ARGS                                                                                             \
  const int64_t *w_ptrs, const int64_t *g_ptrs, const int64_t *key_numel, const int64_t *key_offset, int64_t n_keys, \
      void *state, int64_t state_elems, const double *coef, int first, int form, double *partials,                  \
      int64_t partial_elems, double *stats, void *host_ws, void *dev_ws, int64_t ws_bytes, void *stream
#define FEDAVG_ADAM_PASS                                                                                          \
  w_ptrs, g_ptrs, key_numel, key_offset, n_keys, state, state_elems, coef, first, form, partials, partial_elems, \
      stats, host_ws, dev_ws, ws_bytes, stream

extern "C" {

int fedavg_clientadam_abi_version(void) { return 1; }

const char* fedavg_clientadam_last_error(void) { return g_ca_err.c_str(); }

int64_t fedavg_client_adam_span(int64_t elem_size) { return client_span(elem_size); }

int64_t fedavg_client_adam_workspace(int64_t n_keys) { return adam_workspace(n_keys); }

int64_t fedavg_client_adam_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  return client_partials(key_numel, n_keys, client_span(elem_size));
}

int fedavg_client_adam_step_f32(FEDAVG_ADAM_ARGS) {
  return client_adam_step<CaF32>("fedavg_client_adam_step_f32", FEDAVG_ADAM_PASS);
}

int fedavg_client_adam_step_bf16(FEDAVG_ADAM_ARGS) {
  return client_adam_step<CaHalf<BF16Pk>>("fedavg_client_adam_step_bf16", FEDAVG_ADAM_PASS);
}

int fedavg_client_adam_step_f16(FEDAVG_ADAM_ARGS) {
  return client_adam_step<CaHalf<F16Pk>>("fedavg_client_adam_step_f16", FEDAVG_ADAM_PASS);
}

int fedavg_client_adam_step_f64(FEDAVG_ADAM_ARGS) {
  return client_adam_step<CaF64>("fedavg_client_adam_step_f64", FEDAVG_ADAM_PASS);
}

}  // extern "C"
