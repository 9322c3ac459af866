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
// The pass is client_pass.hpp's, with w and g as the key's two sides; the step
// of each dtype, the kernel's body and an entry point's checks are
// client_step_rules.hpp's (shared with the gated step of
// fedavg_client_loop.hip); this file holds the kernels' entry points and the
// C ABI.
#include "client_step_rules.hpp"

#include "fedavg_amd_clientstep.h"

namespace {

thread_local ErrorState g_cs_err;

int cs_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cs_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int cs_launch_status(const char* what) { return launch_status(g_cs_err, what); }

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

// this library's launches: the step as it is, stats = 0 by a memset where there is nothing to step
struct PlainStep {
  int empty(const char* what, double* stats, hipStream_t s) const { return zero_stats(kLib, what, stats, s); }
  int memory(const char*) const { return FEDAVG_OK; }
  template <class T>
  void step(int form, const StepKey* keys, int64_t n_keys, typename T::op alpha, double* partials, int64_t units,
            hipStream_t s) const {
    hipLaunchKernelGGL((form ? client_sgd_step_kernel<T, 1> : client_sgd_step_kernel<T, 0>),
                       dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, keys, n_keys, alpha, partials, units);
  }
  void finalize(const double* partials, int64_t units, double* stats, hipStream_t s) const {
    hipLaunchKernelGGL(client_sgd_step_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, units, stats);
  }
};

template <class T, class... Args>
int client_sgd_step(const char* what, Args... args) {
  return sgd_step_entry<T>(kLib, PlainStep{}, what, args...);
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
