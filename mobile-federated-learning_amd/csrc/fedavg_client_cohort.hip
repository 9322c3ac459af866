// fedavg_client_cohort.hip -- libfedavg_amd_clientcohort.so (include/
// fedavg_amd_clientcohort.h): the local loops of ALL the linear clients of a
// round (fedavg_trainer.py:172-199) in one launch, one workgroup per client.
//
// Each workgroup is the streamed loop of fedavg_client_stream.hip
// (client_stream_core.hpp holds it as a device function): groups of R rows
// through two LDS buffers, direct global-to-LDS row loads, the 16x16x4 fp32
// matrix instructions for both products, every reduction in the same order.
// What is this unit's own:
//
//   One client per CU, many CUs.  Workgroup g reads entry g of the client table
//   (pinned host memory, read where it lies: one uniform 32-B load) and walks
//   its own ceil(B_g / R) groups after checking its own labels.  512 threads at
//   256 registers and up to 150 KiB of LDS: one workgroup fills a CU, and the
//   hardware starts the entries in order, so the caller puts the longest batch
//   first.  The dynamic LDS is sized once for the launch: two buffers if any
//   client has more than R samples, else one.
//
//   Source and destination apart.  Every workgroup loads the parameters from
//   the same global model (served from L2 after the first) and writes them to
//   row `entry.row` of the packed [K, ld] buffer that the reduce kernels read:
//   always, so no row is left uninitialised -- after a tripped guard the
//   parameters as they stood, after a bad label a copy of the model.  A client's
//   bad label or NaN touches no other client.
//
//   One instance per launch for the loads: rows go straight to LDS when
//   D % 4 == 0 and every client's x is 16-B aligned, else the whole launch
//   stages through registers.  The bits do not depend on which.
//
// Row k and record k are, bit for bit, what fedavg_client_linear_stream_f32
// leaves when run alone on client k from the same model.
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <bitset>

#include "client_stream_core.hpp"
#include "fedavg_amd_clientcohort.h"

namespace {

thread_local ErrorState g_co_err;

int co_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_co_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kCohMaxK = 4096;   // a choice: the table is 128 KiB and the records 256 KiB at most
constexpr int kCohMaxB = 16384;  // the stream library's: B * D <= 2^24, every element index fits 32 bits
static_assert(static_cast<int64_t>(kCohMaxB) * kLinMaxD <= (int64_t{1} << 24), "32-bit indexing");

// rows per group and floats per LDS row: the stream library's arithmetic (fedavg_client_stream_group_rows)
int64_t coh_row_floats(int64_t D) { return 4 * ((D + 3) / 4) + 4; }
int64_t coh_group_rows(int64_t D) {
  for (int64_t r = kLinMaxB; r > 16; r >>= 1)
    if (2 * r * coh_row_floats(D) * 4 <= kLinResidentBytes) return r;
  return 16;
}

// an entry of the client table, as the header lays it out
struct CohEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t row;
};
static_assert(sizeof(CohEntry) == 32, "the header's 32-B entry");

struct CohArgs {
  const float* model;
  float* rows;
  const CohEntry* clients;
  const double* coef;
  double* rec;
  int64_t ld;
  double lr_ratio;
  float alpha;
  int D, C, iters, act, form, R;
};

template <bool ADAM, bool DMA>
__global__ __launch_bounds__(kLinThreads) void client_cohort_f32_kernel(const CohArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // one or two buffers of R rows of S floats
  const CohEntry e = a.clients[blockIdx.x];                   // uniform: the workgroup's own client
  const int P0 = a.C * a.D;
  float* row = a.rows + e.row * a.ld;
  const StrClient c = {a.model, a.model + P0, row, row + P0, e.x, e.y, a.coef, a.rec + 8 * e.row, a.lr_ratio, a.alpha,
                       static_cast<int>(e.B), a.D, a.C, a.iters, a.act, a.form, a.R};
  str_client_loop<ADAM, DMA>(c, xs);
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

template <bool ADAM, bool DMA>
int coh_launch(const char* what, const CohArgs& a, int64_t K, int64_t lds, hipStream_t s) {
  const auto kernel = client_cohort_f32_kernel<ADAM, DMA>;
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return co_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(K)), dim3(kLinThreads), static_cast<size_t>(lds), s, a);
  return launch_status(g_co_err, what);
}

}  // namespace

extern "C" {

int fedavg_clientcohort_abi_version(void) { return 1; }

const char* fedavg_clientcohort_last_error(void) { return g_co_err.c_str(); }

void fedavg_client_cohort_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c) {
  if (max_k) *max_k = kCohMaxK;
  if (max_b) *max_b = kCohMaxB;
  if (max_d) *max_d = kLinMaxD;
  if (max_c) *max_c = kLinMaxC;
}

int fedavg_client_cohort_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K, int64_t D,
                             int64_t C, int64_t iters, int activation, int optimizer, double lr, double lr_ratio,
                             int form, const double* coef, double* rec, void* stream) {
  const char* what = "fedavg_client_cohort_f32";
  if (!model || !rows || !clients || !rec) return co_error(FEDAVG_EINVAL, "%s: null model, rows, clients or rec", what);
  if (K < 1 || K > kCohMaxK) return co_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kCohMaxK);
  if (D < 1 || D > kLinMaxD) return co_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return co_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  const int64_t P = C * D + C;
  if (ld < P) return co_error(FEDAVG_EINVAL, "%s: ld = %lld below P = %lld", what, (long long)ld, (long long)P);
  if (iters < 0 || iters > INT32_MAX) return co_error(FEDAVG_EINVAL, "%s: negative iteration count", what);
  if (activation != 0 && activation != 1)
    return co_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return co_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return co_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && iters > 0 && !coef) return co_error(FEDAVG_EINVAL, "%s: null coef", what);
  if (misaligned(model, 4) || misaligned(rows, 4) || misaligned(clients, 8) || misaligned(rec, 8) ||
      (adam && misaligned(coef, 8)))
    return co_error(FEDAVG_EALIGN, "%s: model, rows must be 4-B, clients, rec and coef 8-B aligned", what);

  // ---- the table, read on the host where it lies
  const CohEntry* tab = static_cast<const CohEntry*>(clients);
  const int64_t R = coh_group_rows(D);
  std::bitset<kCohMaxK> seen;
  bool two = false, dma = D % 4 == 0;
  for (int64_t g = 0; g < K; ++g) {
    const CohEntry& e = tab[g];
    if (!e.x || !e.y) return co_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kCohMaxB)
      return co_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kCohMaxB);
    if (e.row < 0 || e.row >= K)
      return co_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld outside [0, %lld)", what, (long long)g, (long long)e.row,
                      (long long)K);
    if (seen[e.row]) return co_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld used twice", what, (long long)g, (long long)e.row);
    seen[e.row] = true;
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return co_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    two = two || e.B > R;
    dma = dma && !misaligned(e.x, 16);
  }

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return co_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || !is_device_memory(rows))
    return co_error(FEDAVG_EINVAL, "%s: model and rows must be device memory", what);
  if (!is_device_memory(rec) && !is_pinned_host_memory(rec))
    return co_error(FEDAVG_EINVAL, "%s: rec must be device or pinned host memory", what);
  if (adam && iters > 0) {
    if (!is_pinned_host_memory(coef)) return co_error(FEDAVG_EINVAL, "%s: coef is not pinned host memory", what);
    for (int64_t t = 0; t < iters; ++t)
      if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
        return co_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                        coef[kAdamCoefs * t + 1]);
  }
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return co_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  const CohArgs a = {model, rows, tab, coef, rec, ld, lr_ratio, static_cast<float>(-lr),  // ATen: rounded once to opmath
                     static_cast<int>(D), static_cast<int>(C), static_cast<int>(iters), activation, form,
                     static_cast<int>(R)};
  const int64_t lds = (two ? 2 : 1) * R * coh_row_floats(D) * 4;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dma) return adam ? coh_launch<true, true>(what, a, K, lds, s) : coh_launch<false, true>(what, a, K, lds, s);
  return adam ? coh_launch<true, false>(what, a, K, lds, s) : coh_launch<false, false>(what, a, K, lds, s);
}

}  // extern "C"
