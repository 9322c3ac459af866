// fedavg_client_vec.hip -- libfedavg_amd_clientvec.so (include/
// fedavg_amd_clientvec.h): the client's per-iteration statistics in one pass
// for bf16, fp16 and fp64 models.
//
// client_pass.hpp's statistics pass with these rules.  Per element of type T
// it forms
//     d = rT(f32(cur) - f32(snap))   bf16 / fp16: the difference in T (:78)
//     d = cur - snap                 fp64
//     sum cur^2, sum d^2             (squares and sums in fp64)
//     count of isnan(cur)
//     snap = cur                     (the bits, NaN payloads included)
// moving 6 B per 16-bit element and 24 B per fp64 element (read cur, read
// snap, write snap).  fedavg_client_track_{bf16,f16,f64} keep the running
// rho / beta of :78-84 on the device in the model's type.
#include "client_pass.hpp"

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

// ---------------------------------------------------------------------------
// Dtype rules: what one slice adds to {NaN count, sum cur^2, sum d^2}.
// ---------------------------------------------------------------------------
// bf16 / fp16; R = BF16Pk / F16Pk (common.hpp): two elements per 32-bit word
template <class R>
struct CvHalf : CliElem<2> {
  typedef CliOpHalf<R> scalar;
  template <bool HAS>
  __device__ static void add(const CliSlice& c, const CliSlice& s, int& nans, double& a_cur, double& a_d) {
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
};

struct CvF64 : CliElem<8> {
  typedef CliOpF64 scalar;
  template <bool HAS>
  __device__ static void add(const CliSlice& c, const CliSlice& s, int& nans, double& a_cur, double& a_d) {
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

template <class T, bool HAS>
__global__ __launch_bounds__(kBlock) void clientvec_stats_kernel(const ClientKey* __restrict__ keys, int64_t n_keys,
                                                                 typename T::elem* __restrict__ snap,
                                                                 double* __restrict__ partials, int64_t units) {
  cli_stats_pass<T, HAS>(keys, n_keys, snap, partials, units);
}

__global__ __launch_bounds__(kBlock) void clientvec_finalize_kernel(const double* __restrict__ partials, int64_t units,
                                                                    double* __restrict__ stats) {
  cli_finalize(partials, units, stats);
}

// client.py:78-84 on the device in the model's type (client_pass.hpp's cli_track)
template <class T>
__global__ __launch_bounds__(64) void clientvec_track_kernel(double* __restrict__ state,
                                                             const double* __restrict__ w_stats,
                                                             const double* __restrict__ g_stats, double abs_dloss) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  cli_track<typename T::scalar>(state, w_stats, g_stats, abs_dloss);
}

int bad_tensor(const char* what, int64_t key, int64_t elem_size) {
  return cv_error(FEDAVG_EINVAL, "%s: key %lld: null tensor or address not a multiple of %lld bytes", what,
                  (long long)key, (long long)elem_size);
}

const ClientLib kLib = {cv_error, cv_launch_status, clientvec_finalize_kernel, bad_tensor};

// this library has no fp32 pass (that one is libfedavg_amd.so's)
int64_t span_of(int64_t elem_size) { return elem_size == 2 || elem_size == 8 ? client_span(elem_size) : 0; }

// the entry points of rule T: the shared host code with this library's kernels
template <class T, class... Args>
int client_stats_vec(const char* what, Args... args) {
  return client_stats_entry<T>(kLib, what, {clientvec_stats_kernel<T, false>, clientvec_stats_kernel<T, true>},
                               args...);
}

template <class T, class... Args>
int client_track_vec(const char* what, Args... args) {
  return client_track_entry(kLib, what, clientvec_track_kernel<T>, args...);
}

}  // namespace

extern "C" {

int fedavg_clientvec_abi_version(void) { return 1; }

const char* fedavg_clientvec_last_error(void) { return g_cv_err.c_str(); }

int64_t fedavg_client_stats_vec_span(int64_t elem_size) { return span_of(elem_size); }

int64_t fedavg_client_stats_vec_workspace(int64_t n_keys) { return client_workspace(n_keys); }

int64_t fedavg_client_stats_vec_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size) {
  return client_partials(key_numel, n_keys, span_of(elem_size));
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
