// fedavg_client_loop.hip -- libfedavg_amd_clientloop.so (include/
// fedavg_amd_clientloop.h): a local iteration of Client.train (client.py:69-86)
// that never stops the host, for fp32, bf16 and fp64 models.
//
// With the statistics and the step on the device, the one thing left on the
// host was the :71 guard: read the records back, compare two norms, decide
// whether the optimizer steps.  Here
//   client_guard_kernel      decides :71 from the records where they lie and
//                            sets a sticky gate {gate, trip epoch};
//   client_*_step_gated_kernel   is the SGD / Adam step of
//                            client_step_rules.hpp / client_adam_rules.hpp,
//                            every workgroup reading the gate first (a uniform
//                            value) and returning when it is set;
//   client_loop_finalize_kernel  reads the gate too, adds the partials up as
//                            every client library's finalize does and then
//                            does the track update of :78-84 (client_pass.hpp's
//                            cli_track) with |loss - last_loss| formed here
//                            from the record's two loss slots: no separate
//                            track launch.
// A set gate leaves every byte the step would have written as it was, so the
// host may run ahead and read ONE record at the end of the loop.
//
// The arithmetic of the steps exists once, in the two rules headers; this
// file holds the guard, the gated entry points and the C ABI.
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include "fedavg_amd_clientloop.h"

namespace {

thread_local ErrorState g_cl_err;

int cl_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cl_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int cl_launch_status(const char* what) { return launch_status(g_cl_err, what); }

// ---------------------------------------------------------------------------
// The guard.  Op: the scalar arithmetic of the model's type (client_pass.hpp).
// Every fp32 operation is formed in fp64 from fp32 operands and rounded once
// to fp32, as cli_track forms them.
// ---------------------------------------------------------------------------
template <class Op>
__device__ __forceinline__ double guard_norm(double sumsq) {
  const double r = __builtin_sqrt(sumsq);  // a NaN sum gives a NaN norm
  if constexpr (Op::kF64) return r;
  return Op::rt(static_cast<float>(r));
}

// lr * ratio * norm(last_w): python_float * tensor, the scalar rounded to opmath, the product to the tensor's type
template <class Op>
__device__ __forceinline__ double guard_bound(double n_w, double lr_ratio) {
  if constexpr (Op::kF64) return n_w * lr_ratio;
  const double s = static_cast<double>(static_cast<float>(lr_ratio));
  return Op::rt(static_cast<float>(s * n_w));  // the fp64 product of two fp32 values is exact: one rounding
}

template <class Op>
__global__ __launch_bounds__(64) void client_guard_kernel(const double* rec_g, const double* rec_w,
                                                          const double* loss, double* gate, double lr_ratio,
                                                          double epoch) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (gate[0] != 0.0) return;  // sticky: the first trip stays
  const double n_g = guard_norm<Op>(rec_g[1]), n_w = guard_norm<Op>(rec_w[1]);
  const double bound = guard_bound<Op>(n_w, lr_ratio);
  const double l = *loss;
  if (rec_g[0] > 0.0 || l != l || n_g > bound) {
    gate[0] = 1.0;
    gate[1] = epoch;
  }
}

// ---------------------------------------------------------------------------
// The gated launches
// ---------------------------------------------------------------------------
template <class T, int FORM>
__global__ __launch_bounds__(kBlock) void client_sgd_step_gated_kernel(const double* gate,
                                                                       const StepKey* __restrict__ keys,
                                                                       int64_t n_keys, typename T::op alpha,
                                                                       double* __restrict__ partials, int64_t units) {
  if (*gate != 0.0) return;  // uniform over the launch
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

template <class T, bool FIRST>
__global__ __launch_bounds__(kBlock) void client_adam_step_gated_kernel(
    const double* gate, const AdamKey* __restrict__ keys, int64_t n_keys, typename T::elem* __restrict__ state,
    int64_t plane, typename T::op wd, typename T::op lw, typename T::op beta2, typename T::op value,
    typename T::op bc2s, typename T::op eps, typename T::op step, int form, int has_wd,
    double* __restrict__ partials, int64_t units) {
  if (*gate != 0.0) return;  // uniform over the launch
  const AdamCoef<typename T::op> c = {wd, lw, beta2, value, bc2s, eps, step, form, has_wd};
  adam_step_pass<T, FIRST>(keys, n_keys, state, plane, c, partials, units);
}

// one workgroup: stats = the partials' sums (units == 0: zeros), then :78-84 and loss[1] = loss[0]
template <class Op>
__global__ __launch_bounds__(kBlock) void client_loop_finalize_kernel(const double* gate,
                                                                      const double* __restrict__ partials,
                                                                      int64_t units, double* stats,
                                                                      const double* g_stats, double* state,
                                                                      double* loss) {
  if (*gate != 0.0) return;
  cli_finalize(partials, units, stats);
  if (threadIdx.x == 0) {  // the thread that wrote stats
    const double l = loss[0];
    cli_track<Op>(state, stats, g_stats, __builtin_fabs(l - loss[1]));
    loss[1] = l;
  }
}

int bad_tensor(const char* what, int64_t key, int64_t elem_size) {
  return cl_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                  (long long)key, (long long)elem_size);
}

// the shared host code launches the finalize through GatedStep below, never through this table
const ClientLib kLib = {cl_error, cl_launch_status, nullptr, bad_tensor};

bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// what a gated entry adds to its step's arguments, and this library's launches
template <class Op>
struct GatedStep {
  const double* g_stats;
  const double* gate;
  double* state;
  double* loss;

  // before anything else, and before any HIP call
  int check(const char* what) const {
    if (!g_stats || !gate || !state || !loss)
      return cl_error(FEDAVG_EINVAL, "%s: null g_stats, gate, state or loss", what);
    if (misaligned8(g_stats) || misaligned8(gate) || misaligned8(state) || misaligned8(loss))
      return cl_error(FEDAVG_EALIGN, "%s: g_stats, gate, state and loss must be 8-B aligned", what);
    return FEDAVG_OK;
  }
  int memory(const char* what) const {
    if (!is_device_memory(g_stats) || !is_device_memory(gate) || !is_device_memory(state) || !is_device_memory(loss))
      return cl_error(FEDAVG_EINVAL, "%s: g_stats, gate, state and loss must be device memory", what);
    return FEDAVG_OK;
  }
  // nothing to step: the finalize alone, over no partials
  int empty(const char* what, double* stats, hipStream_t s) const {
    if (!is_device_memory(stats)) return cl_error(FEDAVG_EINVAL, "%s: stats must be device memory", what);
    if (const int rc = memory(what)) return rc;
    finalize(nullptr, 0, stats, s);
    return cl_launch_status(what);
  }
  template <class T>
  void step(int form, const StepKey* keys, int64_t n_keys, typename T::op alpha, double* partials, int64_t units,
            hipStream_t s) const {
    hipLaunchKernelGGL((form ? client_sgd_step_gated_kernel<T, 1> : client_sgd_step_gated_kernel<T, 0>),
                       dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, gate, keys, n_keys, alpha, partials,
                       units);
  }
  template <class T>
  void step(bool first, const AdamKey* keys, int64_t n_keys, typename T::elem* adam_state, int64_t state_elems,
            const AdamCoef<typename T::op>& c, double* partials, int64_t units, hipStream_t s) const {
    hipLaunchKernelGGL((first ? client_adam_step_gated_kernel<T, true> : client_adam_step_gated_kernel<T, false>),
                       dim3(static_cast<unsigned>(units)), dim3(kBlock), 0, s, gate, keys, n_keys, adam_state,
                       state_elems, c.wd, c.lw, c.beta2, c.value, c.bc2s, c.eps, c.step, c.form, c.has_wd, partials,
                       units);
  }
  void finalize(const double* partials, int64_t units, double* stats, hipStream_t s) const {
    hipLaunchKernelGGL(client_loop_finalize_kernel<Op>, dim3(1), dim3(kBlock), 0, s, gate, partials, units, stats,
                       g_stats, state, loss);
  }
};

template <class T, class... Args>
int sgd_step_gated(const char* what, const double* g_stats, const double* gate, double* state, double* loss,
                   Args... args) {
  const GatedStep<typename T::scalar> gated = {g_stats, gate, state, loss};
  if (const int rc = gated.check(what)) return rc;
  return sgd_step_entry<T>(kLib, gated, what, args...);
}

template <class T, class... Args>
int adam_step_gated(const char* what, const double* g_stats, const double* gate, double* state, double* loss,
                    Args... args) {
  const GatedStep<typename T::scalar> gated = {g_stats, gate, state, loss};
  if (const int rc = gated.check(what)) return rc;
  return adam_step_entry<T>(kLib, gated, what, args...);
}

template <class Op>
int client_guard(const char* what, const double* rec_g, const double* rec_w, const double* loss, double* gate,
                 double lr_ratio, int64_t epoch, void* stream) {
  if (!rec_g || !rec_w || !loss || !gate) return cl_error(FEDAVG_EINVAL, "%s: null argument", what);
  if (epoch < 0) return cl_error(FEDAVG_EINVAL, "%s: negative epoch", what);
  if (misaligned8(rec_g) || misaligned8(rec_w) || misaligned8(loss) || misaligned8(gate))
    return cl_error(FEDAVG_EALIGN, "%s: records must be 8-B aligned", what);
  if (!is_device_memory(rec_g) || !is_device_memory(rec_w) || !is_device_memory(loss) || !is_device_memory(gate))
    return cl_error(FEDAVG_EINVAL, "%s: records must be device memory", what);
  hipLaunchKernelGGL(client_guard_kernel<Op>, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), rec_g, rec_w,
                     loss, gate, lr_ratio, static_cast<double>(epoch));
  return cl_launch_status(what);
}

}  // namespace

#define FEDAVG_GATE_ARGS const double *g_stats, const double *gate, double *state, double *loss
#define FEDAVG_GATE_PASS g_stats, gate, state, loss
#define FEDAVG_SGD_ARGS                                                                                        \
  const int64_t *w_ptrs, const int64_t *g_ptrs, const int64_t *key_numel, int64_t n_keys, double lr, int form, \
      double *partials, int64_t partial_elems, double *stats, void *host_ws, void *dev_ws, int64_t ws_bytes,  \
      void *stream
#define FEDAVG_SGD_PASS \
  w_ptrs, g_ptrs, key_numel, n_keys, lr, form, partials, partial_elems, stats, host_ws, dev_ws, ws_bytes, stream
#define FEDAVG_ADAM_ARGS                                                                                             \
  const int64_t *w_ptrs, const int64_t *g_ptrs, const int64_t *key_numel, const int64_t *key_offset, int64_t n_keys, \
      void *adam_state, int64_t state_elems, const double *coef, int first, int form, double *partials,             \
      int64_t partial_elems, double *stats, void *host_ws, void *dev_ws, int64_t ws_bytes, void *stream
#define FEDAVG_ADAM_PASS                                                                                \
  w_ptrs, g_ptrs, key_numel, key_offset, n_keys, adam_state, state_elems, coef, first, form, partials, \
      partial_elems, stats, host_ws, dev_ws, ws_bytes, stream

extern "C" {

int fedavg_clientloop_abi_version(void) { return 1; }

const char* fedavg_clientloop_last_error(void) { return g_cl_err.c_str(); }

int64_t fedavg_client_loop_span(int64_t elem_size) { return client_span(elem_size); }

int64_t fedavg_client_loop_workspace(int64_t n_keys, int for_adam) {
  return for_adam ? adam_workspace(n_keys) : client_workspace(n_keys);
}

int64_t fedavg_client_loop_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  return client_partials(key_numel, n_keys, client_span(elem_size));
}

int fedavg_client_guard_f32(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                            double lr_ratio, int64_t epoch, void* stream) {
  return client_guard<CliOpF32>("fedavg_client_guard_f32", rec_g, rec_w, loss, gate, lr_ratio, epoch, stream);
}

int fedavg_client_guard_bf16(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                             double lr_ratio, int64_t epoch, void* stream) {
  return client_guard<CliOpHalf<BF16Pk>>("fedavg_client_guard_bf16", rec_g, rec_w, loss, gate, lr_ratio, epoch,
                                         stream);
}

int fedavg_client_guard_f64(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                            double lr_ratio, int64_t epoch, void* stream) {
  return client_guard<CliOpF64>("fedavg_client_guard_f64", rec_g, rec_w, loss, gate, lr_ratio, epoch, stream);
}

int fedavg_client_sgd_step_gated_f32(FEDAVG_SGD_ARGS, FEDAVG_GATE_ARGS) {
  return sgd_step_gated<CsF32>("fedavg_client_sgd_step_gated_f32", FEDAVG_GATE_PASS, FEDAVG_SGD_PASS);
}

int fedavg_client_sgd_step_gated_bf16(FEDAVG_SGD_ARGS, FEDAVG_GATE_ARGS) {
  return sgd_step_gated<CsHalf<BF16Pk>>("fedavg_client_sgd_step_gated_bf16", FEDAVG_GATE_PASS, FEDAVG_SGD_PASS);
}

int fedavg_client_sgd_step_gated_f64(FEDAVG_SGD_ARGS, FEDAVG_GATE_ARGS) {
  return sgd_step_gated<CsF64>("fedavg_client_sgd_step_gated_f64", FEDAVG_GATE_PASS, FEDAVG_SGD_PASS);
}

int fedavg_client_adam_step_gated_f32(FEDAVG_ADAM_ARGS, FEDAVG_GATE_ARGS) {
  return adam_step_gated<CaF32>("fedavg_client_adam_step_gated_f32", FEDAVG_GATE_PASS, FEDAVG_ADAM_PASS);
}

int fedavg_client_adam_step_gated_bf16(FEDAVG_ADAM_ARGS, FEDAVG_GATE_ARGS) {
  return adam_step_gated<CaHalf<BF16Pk>>("fedavg_client_adam_step_gated_bf16", FEDAVG_GATE_PASS, FEDAVG_ADAM_PASS);
}

int fedavg_client_adam_step_gated_f64(FEDAVG_ADAM_ARGS, FEDAVG_GATE_ARGS) {
  return adam_step_gated<CaF64>("fedavg_client_adam_step_gated_f64", FEDAVG_GATE_PASS, FEDAVG_ADAM_PASS);
}

}  // extern "C"
