// fedavg_client_split.hip -- libfedavg_amd_clientsplit.so (include/
// fedavg_amd_clientsplit.h): central_train's chain of optimizer steps
// (fedavg_trainer.py:361-371) for a linear softmax model with each step's batch
// split across workgroups.  The chain of fedavg_client_chain.hip is one
// persistent workgroup, so a step's rows pass through one CU; the steps of a
// chain depend on each other, the rows inside a step do not.  Here a step is
// two launches in stream order and nothing else orders them:
//
//   The gradient launch, one workgroup per slice of R rows.  R is the most rows
//   of S = D4 + 4 floats that fit the streamed loop's LDS budget in ONE buffer
//   (there is nothing to overlap a second one with: a workgroup has one slice),
//   in multiples of 16 up to 256.  The slice goes into LDS once (str_fetch of
//   client_stream_core.hpp: global memory to LDS directly, or staged), W and b
//   come from global memory (L2 after the first workgroup) into the registers in
//   which the 16x16x4 matrix instruction consumes W.  The slice is walked in
//   sub-groups of 64 rows: the waves split the D columns, their partial logits
//   meet in LDS, one thread per row runs lin_sample with 1 / B of the WHOLE
//   batch, and dW += dz^T x with dz^T as A (classes down the 16 rows) and the
//   LDS-resident x as B (16 columns of the wave's tile across): a lane's four
//   results are four classes of one column, so the 16 lanes of a quarter-wave
//   store 64 contiguous bytes of a row of the slot's dW.  Slot g of the plane
//   [G, P] takes the partial dW and db, lsum[g] the slice's fp64 loss sum in
//   sample order.
//
//   The step launch, one thread per four parameters.  It adds the G slots of
//   its parameters in slot order in fp32 and puts them through lin_step
//   (client_linear_core.hpp), W, b and Adam's m, v, vmax in global memory.
//   Thread 0 of workgroup 0 adds lsum in slot order and writes the loss where
//   the chain writes it.
//
//   The label launch, once, before the first step: one workgroup, the table
//   512 entries at a time through LDS as in the chain; head[0] = 1 and rec name
//   the lowest entry with a label outside [0, C).  Every later launch reads
//   head[0] first and returns if it is set.
//
// Workspace: head (256 B: word 0 the label flag), lsum [Gmax] fp64, plane
// [Gmax, P] fp32, Gmax = ceil(the table's largest B / R).
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <climits>

#include "client_stream_core.hpp"
#include "fedavg_amd_clientsplit.h"

namespace {

thread_local ErrorState g_sp_err;

int sp_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_sp_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kSpMaxK = 4096, kSpMaxB = 16384;  // the chain's ranges
static_assert(static_cast<int64_t>(kSpMaxB) * kLinMaxD <= (int64_t{1} << 24), "32-bit indexing");
constexpr int kSpMaxR = 4 * kLinMaxB;         // rows of a slice: at most four sub-groups
constexpr int kSpStepThreads = 256;           // the step launch: four parameters a thread
constexpr int kSpLabelChunk = kLinThreads;    // table entries checked per pass of the label check
constexpr int64_t kSpHeadBytes = 256;         // the workspace's head: word 0 is the label flag

int64_t sp_row_floats(int64_t D) { return 4 * ((D + 3) / 4) + 4; }
int64_t sp_slice_rows(int64_t D) {
  const int64_t r = 16 * (kLinResidentBytes / (16 * sp_row_floats(D) * 4));
  return r > kSpMaxR ? kSpMaxR : r;
}
static_assert(kLinResidentBytes >= 32 * (kLinMaxD + 4) * 4, "two row tiles at the widest D");
int64_t sp_slices(int64_t B, int64_t D) { return (B + sp_slice_rows(D) - 1) / sp_slice_rows(D); }
int64_t sp_workspace(int64_t max_b, int64_t D, int64_t C) {
  const int64_t G = sp_slices(max_b, D), P = C * D + C;
  return kSpHeadBytes + 8 * G + 4 * G * P;
}

// an entry of the client table, as the chain's header lays it out
struct SpEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t unused;
};
static_assert(sizeof(SpEntry) == 32, "the header's 32-B entry");

// ---------------------------------------------------------------- every label of every entry, once
__global__ __launch_bounds__(kLinThreads) void client_split_labels_kernel(const SpEntry* clients, int K, int C,
                                                                          int* head, double* rec) {
  __shared__ SpEntry tab[kSpLabelChunk];
  __shared__ int bads[kLinThreads];
  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63;
  int bad = INT_MAX;
  for (int k0 = 0; k0 < K; k0 += kSpLabelChunk) {
    __syncthreads();  // the chunk before this one has been walked
    if (k0 + tid < K) tab[tid] = clients[k0 + tid];
    __syncthreads();
    const int n = K - k0 < kSpLabelChunk ? K - k0 : kSpLabelChunk;
    for (int j = wave; j < n; j += kLinWaves) {
      const int64_t* y = tab[j].y;
      const int B = static_cast<int>(tab[j].B);
      for (int b = lane; b < B; b += 64) {
        const int64_t v = y[b];
        if ((v < 0 || v >= C) && k0 + j < bad) bad = k0 + j;
      }
    }
  }
  bads[tid] = bad;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < kLinThreads; ++t) bad = bads[t] < bad ? bads[t] : bad;
    head[0] = bad != INT_MAX ? 1 : 0;
    head[1] = bad;
    if (bad != INT_MAX) {
      rec[0] = 1.0;
      rec[1] = static_cast<double>(bad);
#pragma unroll
      for (int j = 2; j < 8; ++j) rec[j] = 0.0;
    }
  }
}

// ---------------------------------------------------------------- one slice's partial gradient
struct SpGrad {
  const float* model;
  const float* x;
  const int64_t* y;
  const int* head;
  double* lsum;
  float* plane;
  int B, D, C, R, act;
};

template <bool DMA>
__global__ __launch_bounds__(kLinThreads) void client_split_grad_kernel(const SpGrad a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // the slice: R rows of S floats
  __shared__ float part[kLinWaves / 2][kLinMaxB][16];         // the sub-group's partial logits
  __shared__ float dzs[kLinMaxB][16];                         // the sub-group's dz; rows past its end are 0
  __shared__ float lossb[kLinMaxB];
  __shared__ int corr[kLinMaxB];  // lin_sample's; not reported
  __shared__ float bias[16];

  if (a.head[0] != 0) return;  // a bad label: nothing is read or written

  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i0 = lane & 15, q0 = lane >> 4;
  const int B = a.B, D = a.D, C = a.C, R = a.R, D4 = (D + 3) & ~3, S = D4 + 4, P0 = C * D, P = P0 + C;
  const int g = static_cast<int>(blockIdx.x), row0 = g * R, rows = B - row0 < R ? B - row0 : R;

  // ---- the slice sets out for LDS; rows from B on are never read
  str_fetch<DMA>(a.x, xs, row0, rows, D, D4, S);

  // ---- W as the forward's B operand, b for the samples
  float wv[kLinSlots][4];
  f32x4 ga[kLinSlots];  // the slice's dW: ga[k][r] is class 4 q + r, column 16 (kLinWaves k + wave) + i
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q0;
    ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = i0 < C && d0 + r < D;
      const float w = a.model[on ? i0 * D + d0 + r : 0];
      wv[k][r] = on ? w : 0.f;
    }
  }
  if (tid < 16) {
    const float bw = a.model[P0 + (tid < C ? tid : 0)];
    bias[tid] = tid < C ? bw : 0.f;
  }
  const float inv_b = 1.0f / static_cast<float>(B);
  double loss_sum = 0.0;  // thread 0's, in sample order across the sub-groups
  float db = 0.f;         // thread c's sum of dz[., c], in sample order across the sub-groups
  if constexpr (DMA) str_landed();

  for (int s0 = 0; s0 < rows; s0 += kLinMaxB) {
    const int i = lin_opaque(i0), q = lin_opaque(q0);
    const int srows = rows - s0 < kLinMaxB ? rows - s0 : kLinMaxB;
    const int MT = (srows + 15) >> 4, KS = (srows + 3) >> 2;
    // ---- the slice and the bias are in LDS (first pass); no wave still reads part or dzs (later ones)
    __syncthreads();
    const LinBatch<true> xb = {xs + s0 * S, a.x, srows, D, D4, S};

    // ---- forward: this wave's part of z = x W^T for the sub-group's row tiles
    f32x4 z[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) z[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int n0 = 16 * (kLinWaves * k + wave);
      if (n0 < D) {
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          if (mt < MT) {
            const f32x4 xa = xb.row4(16 * mt + i, n0 + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) z[mt] = mfma4(xa[r], wv[k][r], z[mt]);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // a tile at a time: no tile's loads wait in registers behind another's
    }
    if (wave >= kLinWaves / 2) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[wave - kLinWaves / 2][16 * mt + 4 * q + r][i] = z[mt][r];
    }
    __syncthreads();
    if (wave < kLinWaves / 2) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float* p = &part[wave][16 * mt + 4 * q + r][i];
          *p = z[mt][r] + *p;
        }
    }
    __syncthreads();

    // ---- one thread per row of the sub-group; the rows past its end leave zero dz
    if (tid < srows) {
      const int64_t y = a.y[row0 + s0 + tid];  // checked by the label launch; compared, never an index
      lin_sample(part, bias, dzs, tid, static_cast<int>(y), C, a.act, inv_b, lossb[tid], corr[tid]);
    } else if (tid < kLinMaxB) {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) dzs[tid][cc] = 0.f;
    }
    __syncthreads();

    // ---- the loss by thread 0, db by thread c, the tiles' dz^T x: all in sample order
    if (tid == 0)
      for (int b = 0; b < srows; ++b) loss_sum += static_cast<double>(lossb[b]);
    if (tid < 16)
      for (int b = 0; b < srows; ++b) db += dzs[b][tid];
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int n0 = 16 * (kLinWaves * k + wave);
      if (n0 < D) {
        for (int ks = 0; ks < KS; ++ks) ga[k] = mfma4(dzs[4 * ks + q][i], xb.at(4 * ks + q, n0 + i), ga[k]);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- slot g: the slice's dW, db and loss sum, and nothing else
  float* slot = a.plane + static_cast<int64_t>(g) * P;
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d = 16 * (kLinWaves * k + wave) + i0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * q0 + r < C && d < D) slot[(4 * q0 + r) * D + d] = ga[k][r];
  }
  if (tid < C) slot[P0 + tid] = db;
  if (tid == 0) a.lsum[g] = loss_sum;
}

// ---------------------------------------------------------------- the slots' sum and the step
struct SpStep {
  float* model;
  float* state;
  const int* head;
  const double* lsum;
  const float* plane;
  const double* coef;  // Adam: this step's row
  double* loss_out;    // the round's entry of losses, or null
  double* rec;         // on the call's last step, else null
  float alpha;
  int P, G, B, form, carried, total;
};

template <bool ADAM>
__global__ __launch_bounds__(kSpStepThreads) void client_split_step_kernel(const SpStep a) {
  __shared__ double crow[8];
  if (a.head[0] != 0) return;
  const int tid = static_cast<int>(threadIdx.x), P = a.P, G = a.G;
  const int j0 = 4 * (static_cast<int>(blockIdx.x) * kSpStepThreads + tid);
  if constexpr (ADAM) {
    if (tid < kAdamCoefs) crow[tid] = a.coef[tid];
    __syncthreads();
  }
  const int left = P - j0, live = left < 0 ? 0 : left > 4 ? 4 : left;
  if (live > 0) {
    float w4[4], g4[4], m4[4], v4[4], x4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = r < live;
      const int j = on ? j0 + r : j0;
      float s = a.plane[j];
      for (int g = 1; g < G; ++g) s += a.plane[static_cast<int64_t>(g) * P + j];  // slot order
      g4[r] = on ? s : 0.f;
      const float w = a.model[j];
      w4[r] = on ? w : 0.f;
      m4[r] = v4[r] = x4[r] = 0.f;
      if constexpr (ADAM) {
        if (a.carried && on) m4[r] = a.state[j], v4[r] = a.state[P + j], x4[r] = a.state[2 * P + j];
      }
    }
    AdamCoef<float> co = {};
    if constexpr (ADAM)
      co = {static_cast<float>(crow[0]), static_cast<float>(crow[1]), static_cast<float>(crow[2]),
            static_cast<float>(crow[3]), static_cast<float>(crow[4]), static_cast<float>(crow[5]),
            static_cast<float>(crow[6]), a.form, crow[0] != 0.0 ? 1 : 0};
    double wst[2] = {0.0, 0.0};  // the step rules' statistics: not kept here
    int wn = 0;
    lin_step<ADAM>(w4, g4, m4, v4, x4, a.alpha, a.form, co, live, wn, wst[0], wst[1]);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (r < live) {
        a.model[j0 + r] = w4[r];
        if constexpr (ADAM) a.state[j0 + r] = m4[r], a.state[P + j0 + r] = v4[r], a.state[2 * P + j0 + r] = x4[r];
      }
  }
  if (blockIdx.x == 0 && tid == 0 && (a.loss_out || a.rec)) {  // the loss is from before the step: the slots hold it
    double sum = a.lsum[0];
    for (int g = 1; g < G; ++g) sum += a.lsum[g];
    const float loss = static_cast<float>(sum / static_cast<double>(a.B));
    if (a.loss_out) *a.loss_out = static_cast<double>(loss);  // what :372 logs
    if (a.rec) {
      a.rec[0] = 0.0;
      a.rec[1] = -1.0;
      a.rec[2] = static_cast<double>(a.total);
      a.rec[3] = static_cast<double>(loss);
#pragma unroll
      for (int j = 4; j < 8; ++j) a.rec[j] = 0.0;
    }
  }
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int fedavg_clientsplit_abi_version(void) { return 1; }

const char* fedavg_clientsplit_last_error(void) { return g_sp_err.c_str(); }

int64_t fedavg_client_split_slice_rows(int64_t D) { return D < 1 || D > kLinMaxD ? 0 : sp_slice_rows(D); }

int64_t fedavg_client_split_workspace_bytes(int64_t max_B, int64_t D, int64_t C) {
  if (max_B < 1 || max_B > kSpMaxB || D < 1 || D > kLinMaxD || C < 2 || C > kLinMaxC) return 0;
  return sp_workspace(max_B, D, C);
}

int fedavg_client_chain_split_f32(float* model, float* state, const void* clients, int64_t K, int64_t D, int64_t C,
                                  int64_t rounds, int64_t step0, int activation, int optimizer, double lr, int form,
                                  const double* coef, double* losses, double* rec, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  const char* what = "fedavg_client_chain_split_f32";
  if (!model || !clients || !losses || !rec || !workspace)
    return sp_error(FEDAVG_EINVAL, "%s: null model, clients, losses, rec or workspace", what);
  if (K < 1 || K > kSpMaxK) return sp_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kSpMaxK);
  if (D < 1 || D > kLinMaxD) return sp_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return sp_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  if (rounds < 1 || rounds > INT32_MAX / K)
    return sp_error(FEDAVG_EINVAL, "%s: rounds = %lld outside [1, %lld]", what, (long long)rounds,
                    (long long)(INT32_MAX / K));
  if (step0 < 0) return sp_error(FEDAVG_EINVAL, "%s: step0 = %lld is negative", what, (long long)step0);
  if (activation != 0 && activation != 1)
    return sp_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return sp_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return sp_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && !state) return sp_error(FEDAVG_EINVAL, "%s: null state", what);
  if (adam && !coef) return sp_error(FEDAVG_EINVAL, "%s: null coef", what);
  if (misaligned(model, 4) || (adam && misaligned(state, 4)) || misaligned(clients, 8) || misaligned(losses, 8) ||
      misaligned(rec, 8) || (adam && misaligned(coef, 8)) || misaligned(workspace, 8))
    return sp_error(FEDAVG_EALIGN,
                    "%s: model, state must be 4-B, clients, losses, rec, coef and workspace 8-B aligned", what);

  // ---- the table, read on the host where it lies, in its own order
  const SpEntry* tab = static_cast<const SpEntry*>(clients);
  bool dma = D % 4 == 0;
  int64_t max_b = 1;
  for (int64_t g = 0; g < K; ++g) {
    const SpEntry& e = tab[g];
    if (!e.x || !e.y) return sp_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kSpMaxB)
      return sp_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kSpMaxB);
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return sp_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    dma = dma && !misaligned(e.x, 16);
    max_b = e.B > max_b ? e.B : max_b;
  }
  if (workspace_bytes < sp_workspace(max_b, D, C))
    return sp_error(FEDAVG_EINVAL, "%s: workspace of %lld bytes below the %lld of fedavg_client_split_workspace_bytes", what,
                    (long long)workspace_bytes, (long long)sp_workspace(max_b, D, C));

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return sp_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || (adam && !is_device_memory(state)) || !is_device_memory(workspace))
    return sp_error(FEDAVG_EINVAL, "%s: model, state and workspace must be device memory", what);
  for (const double* p : {losses, rec})
    if (!is_device_memory(p) && !is_pinned_host_memory(p))
      return sp_error(FEDAVG_EINVAL, "%s: losses and rec must be device or pinned host memory", what);
  if (adam) {
    if (is_pinned_host_memory(coef)) {
      for (int64_t t = 0; t < rounds * K; ++t)
        if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
          return sp_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                          coef[kAdamCoefs * t + 1]);
    } else if (!is_device_memory(coef)) {
      return sp_error(FEDAVG_EINVAL, "%s: coef must be device or pinned host memory", what);
    }
  }
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return sp_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  const int R = static_cast<int>(sp_slice_rows(D)), P = static_cast<int>(C * D + C);
  const int64_t gmax = sp_slices(max_b, D), lds = R * sp_row_floats(D) * 4;
  int* head = static_cast<int*>(workspace);
  double* lsum = reinterpret_cast<double*>(static_cast<char*>(workspace) + kSpHeadBytes);
  float* plane = reinterpret_cast<float*>(lsum + gmax);
  const auto grad = dma ? client_split_grad_kernel<true> : client_split_grad_kernel<false>;
  const auto step = adam ? client_split_step_kernel<true> : client_split_step_kernel<false>;
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(grad),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return sp_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }

  // ---- 1 + 2 * rounds * K launches, nothing between them but the stream's order
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(client_split_labels_kernel, dim3(1), dim3(kLinThreads), 0, s, tab, static_cast<int>(K),
                     static_cast<int>(C), head, rec);
  const int total = static_cast<int>(rounds * K), step_groups = (P + 4 * kSpStepThreads - 1) / (4 * kSpStepThreads);
  const float alpha = static_cast<float>(-lr);  // ATen: rounded once to opmath
  int t = 0;
  for (int64_t r = 0; r < rounds; ++r) {
    for (int64_t k = 0; k < K; ++k, ++t) {
      const SpEntry& e = tab[k];
      const int B = static_cast<int>(e.B), G = (B + R - 1) / R;
      const SpGrad ga = {model, e.x, e.y, head, lsum, plane, B, static_cast<int>(D), static_cast<int>(C), R, activation};
      hipLaunchKernelGGL(grad, dim3(G), dim3(kLinThreads), static_cast<size_t>(lds), s, ga);
      const SpStep sa = {model, adam ? state : nullptr, head, lsum, plane,
                         adam ? coef + static_cast<int64_t>(kAdamCoefs) * t : nullptr,
                         k + 1 == K ? losses + r : nullptr, t + 1 == total ? rec : nullptr, alpha, P, G, B, form,
                         step0 + t > 0 ? 1 : 0, total};
      hipLaunchKernelGGL(step, dim3(step_groups), dim3(kSpStepThreads), 0, s, sa);
    }
    const int rc = launch_status(g_sp_err, what);  // once a round: a refused launch is not followed by a round of them
    if (rc != FEDAVG_OK) return rc;
  }
  return FEDAVG_OK;
}

}  // extern "C"
