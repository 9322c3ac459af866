// fedavg_client_cosplit.hip -- libfedavg_amd_clientcosplit.so (include/
// fedavg_amd_clientcosplit.h): the local loops of ALL the linear clients of a
// round (fedavg_trainer.py:172-199) with each client's batch split across
// workgroups.  The cohort of fedavg_client_cohort.hip is one persistent
// workgroup per client, so a client's rows pass through one CU epoch after
// epoch and K clients use K CUs; the epochs of a client depend on each other,
// the rows inside an epoch do not, and neither do the clients.  Here a local
// iteration is two launches over all the clients, in stream order, and nothing
// else orders them:
//
//   The setup launch, once, K + 1 workgroups.  Workgroup g < K reads entry g
//   of the pinned table, checks the entry's labels, copies the model into the
//   entry's row, leaves a device copy of the entry, a zeroed state block
//   {label flag, trip epoch or -1, steps, last loss, rho, beta, has rho, has
//   beta} and the record of a client that took no step.  Workgroup K walks the
//   table 512 entries at a time through LDS, gives client k its span {first
//   slot, n_k} and writes the group table: slot first + j is {k, j q}.  Every
//   later launch finds its place there; none reads the pinned table again.
//
//   The gradient launch, one workgroup per slot.  It returns if its client is
//   inert.  W and b come from the client's row into the registers in which the
//   16x16x4 matrix instruction consumes W (fedavg_client_split.hip's layout:
//   dz^T as A, the LDS-resident x as B), the slices of R rows go into LDS one
//   after another through str_fetch, each walked in sub-groups of 64 rows; dW,
//   db, the fp64 loss sum and the correct count run on across the slices in
//   slice and sample order.  ONE LDS buffer: R is the most rows that fit the
//   streamed loop's budget in one buffer, so a second one for the next slice
//   does not fit beside it at this R (at D = 784: 2 x 100,864 B of 163,840 B,
//   beside 21 KiB of static LDS), and halving R to make room would double the
//   slots the step launch sums.  At q > 1 the next slice's loads therefore
//   start when the last sub-group of this one has been read.
//
//   The step launch, one workgroup per client, thread t owning parameters
//   t + 512 j.  It sums the client's slots in slot order in fp32 into
//   registers, forms {NaN count, |g|^2, |g - last_g|^2, |last_w|^2} with
//   lin_block_sum, decides the :71 guard, on a trip records the epoch and
//   leaves the row, else puts the row through lin_step, tracks rho / beta and
//   writes the record when the call ends for the client.  last_g lies in the
//   workspace and is read and replaced by the thread that owns the parameter.
//
// Workspace, for N slots and P parameters: tab [K] 32 B, state [K] 64 B, span
// [K] 8 B, groups [N] 8 B, lc [N, 2] fp64 (loss sum, correct count), last_g
// [K, P], Adam's [K, 3, P] (Adam calls only), plane [N, P].
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <bitset>

#include "client_stream_core.hpp"
#include "fedavg_amd_clientcosplit.h"

namespace {

thread_local ErrorState g_cs_err;

int cs_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cs_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kCsMaxK = 4096, kCsMaxB = 16384;  // the cohort's ranges
static_assert(static_cast<int64_t>(kCsMaxB) * kLinMaxD <= (int64_t{1} << 24), "32-bit indexing");
constexpr int kCsMaxR = 4 * kLinMaxB;  // rows of a slice: at most four sub-groups
constexpr int kCsState = 8;            // doubles of a client's state block
constexpr int kCsScanChunk = kLinThreads;
constexpr int kCsStepSlices = 9;  // the step launch: slices of four parameters per thread
static_assert(4 * kCsStepSlices * kLinThreads >= kLinMaxC * (kLinMaxD + 1), "the step launch holds every parameter");
constexpr int kCsStepAhead = 4;  // the step launch: slots whose loads are in flight together

// the split chain's arithmetic (fedavg_client_split_slice_rows)
int64_t cs_row_floats(int64_t D) { return 4 * ((D + 3) / 4) + 4; }
int64_t cs_slice_rows(int64_t D) {
  const int64_t r = 16 * (kLinResidentBytes / (16 * cs_row_floats(D) * 4));
  return r > kCsMaxR ? kCsMaxR : r;
}
// the workgroups of a client of B rows
int64_t cs_groups(int64_t B, int64_t R, int64_t q) { return ((B + R - 1) / R + q - 1) / q; }
int64_t cs_workspace(int64_t K, int64_t N, int64_t P, bool adam) {
  return 104 * K + 24 * N + 4 * P * (N + K * (adam ? 4 : 1));
}

// an entry of the client table, as the cohort's header lays it out
struct CsEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t row;
};
static_assert(sizeof(CsEntry) == 32, "the header's 32-B entry");

struct CsSpan {
  int first, n;  // a client's slots of the plane
};
struct CsGroup {
  int entry, slice0;  // a slot's client and the first slice of its workgroup
};

struct CsLayout {
  CsEntry* tab;
  double* state;
  CsSpan* span;
  CsGroup* groups;
  double* lc;
  float* last_g;
  float* adam;
  float* plane;
};

CsLayout cs_layout(void* workspace, int64_t K, int64_t N, int64_t P, bool adam) {
  char* p = static_cast<char*>(workspace);
  CsLayout w;
  w.tab = reinterpret_cast<CsEntry*>(p), p += 32 * K;
  w.state = reinterpret_cast<double*>(p), p += 8 * kCsState * K;
  w.span = reinterpret_cast<CsSpan*>(p), p += 8 * K;
  w.groups = reinterpret_cast<CsGroup*>(p), p += 8 * N;
  w.lc = reinterpret_cast<double*>(p), p += 16 * N;
  w.last_g = reinterpret_cast<float*>(p), p += 4 * P * K;
  w.adam = reinterpret_cast<float*>(p), p += adam ? 12 * P * K : 0;
  w.plane = reinterpret_cast<float*>(p);
  return w;
}

// ---------------------------------------------------------------- labels, rows, state, records; the group table
struct CsSetup {
  const float* model;
  float* rows;
  const CsEntry* clients;
  double* rec;
  CsLayout w;
  int64_t ld;
  int K, P, C, R, q;
};

__global__ __launch_bounds__(kLinThreads) void client_cosplit_setup_kernel(const CsSetup a) {
  __shared__ int ns[kCsScanChunk];
  __shared__ int sh_flag;
  const int tid = static_cast<int>(threadIdx.x), g = static_cast<int>(blockIdx.x);
  if (g < a.K) {
    const CsEntry e = a.clients[g];  // uniform: the workgroup's own client
    if (tid == 0) sh_flag = 0;
    __syncthreads();
    const int B = static_cast<int>(e.B);
    for (int b = tid; b < B; b += kLinThreads) {
      const int64_t y = e.y[b];
      if (y < 0 || y >= a.C) sh_flag = 1;
    }
    __syncthreads();
    float* row = a.rows + e.row * a.ld;
    for (int j = tid; j < a.P; j += kLinThreads) row[j] = a.model[j];  // never left uninitialised
    if (tid == 0) {
      const double flag = sh_flag ? 1.0 : 0.0;
      a.w.tab[g] = e;
      double* st = a.w.state + kCsState * g;
      double* rec = a.rec + 8 * e.row;
#pragma unroll
      for (int j = 0; j < 8; ++j) st[j] = rec[j] = 0.0;
      st[0] = flag;
      st[1] = -1.0;
      rec[0] = -1.0;
      rec[5] = flag;
    }
    return;
  }
  int base = 0;  // the slots of the clients before this chunk
  for (int k0 = 0; k0 < a.K; k0 += kCsScanChunk) {
    __syncthreads();  // the chunk before this one has been added up
    const int k = k0 + tid;
    int n = 0;
    if (k < a.K) {
      const int B = static_cast<int>(a.clients[k].B);
      n = ((B + a.R - 1) / a.R + a.q - 1) / a.q;
    }
    ns[tid] = n;
    __syncthreads();
    int first = base;
    for (int t = 0; t < kCsScanChunk; ++t) {
      if (t == tid) first = base;
      base += ns[t];
    }
    if (k < a.K) {
      a.w.span[k] = CsSpan{first, n};
      for (int j = 0; j < n; ++j) a.w.groups[first + j] = CsGroup{k, j * a.q};
    }
  }
}

// ---------------------------------------------------------------- one workgroup's partial gradient
struct CsGrad {
  const float* rows;
  CsLayout w;
  int64_t ld;
  int D, C, R, q, act;
};

template <bool DMA>
__global__ __launch_bounds__(kLinThreads) void client_cosplit_grad_kernel(const CsGrad a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // the slice: R rows of S floats
  __shared__ float part[kLinWaves / 2][kLinMaxB][16];         // the sub-group's partial logits
  __shared__ float dzs[kLinMaxB][16];                         // the sub-group's dz; rows past its end are 0
  __shared__ float lossb[kLinMaxB];
  __shared__ int corr[kLinMaxB];
  __shared__ float bias[16];

  const CsGroup gr = a.w.groups[blockIdx.x];
  const double* st = a.w.state + kCsState * gr.entry;
  if (st[0] != 0.0 || st[1] >= 0.0) return;  // a bad label or a tripped guard: nothing is read or written
  const CsEntry e = a.w.tab[gr.entry];

  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i0 = lane & 15, q0 = lane >> 4;
  const int B = static_cast<int>(e.B), D = a.D, C = a.C, R = a.R, D4 = (D + 3) & ~3, S = D4 + 4, P0 = C * D, P = P0 + C;
  const int G = (B + R - 1) / R, send = gr.slice0 + a.q < G ? gr.slice0 + a.q : G;
  const float* model = a.rows + e.row * a.ld;

  // ---- the first slice sets out for LDS; rows from B on are never read
  {
    const int row0 = gr.slice0 * R;
    str_fetch<DMA>(e.x, xs, row0, B - row0 < R ? B - row0 : R, D, D4, S);
  }

  // ---- W as the forward's B operand, b for the samples
  float wv[kLinSlots][4];
  f32x4 ga[kLinSlots];  // the workgroup's dW: ga[k][r] is class 4 q + r, column 16 (kLinWaves k + wave) + i
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q0;
    ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = i0 < C && d0 + r < D;
      const float w = model[on ? i0 * D + d0 + r : 0];
      wv[k][r] = on ? w : 0.f;
    }
  }
  if (tid < 16) {
    const float bw = model[P0 + (tid < C ? tid : 0)];
    bias[tid] = tid < C ? bw : 0.f;
  }
  const float inv_b = 1.0f / static_cast<float>(B);
  double loss_sum = 0.0;  // thread 0's, in sample order across the slices
  int correct = 0;        // thread 0's
  float db = 0.f;         // thread c's sum of dz[., c], in sample order across the slices

  for (int sl = gr.slice0; sl < send; ++sl) {
    const int row0 = sl * R, rows = B - row0 < R ? B - row0 : R;
    if (sl != gr.slice0) {
      __syncthreads();  // no wave still reads the slice before this one
      str_fetch<DMA>(e.x, xs, row0, rows, D, D4, S);
    }
    if constexpr (DMA) str_landed();

    for (int s0 = 0; s0 < rows; s0 += kLinMaxB) {
      const int i = lin_opaque(i0), q = lin_opaque(q0);
      const int srows = rows - s0 < kLinMaxB ? rows - s0 : kLinMaxB;
      const int MT = (srows + 15) >> 4, KS = (srows + 3) >> 2;
      // ---- the slice and the bias are in LDS (first pass); no wave still reads part or dzs (later ones)
      __syncthreads();
      const LinBatch<true> xb = {xs + s0 * S, e.x, srows, D, D4, S};

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
        const int64_t y = e.y[row0 + s0 + tid];  // checked by the setup launch; compared, never an index
        lin_sample(part, bias, dzs, tid, static_cast<int>(y), C, a.act, inv_b, lossb[tid], corr[tid]);
      } else if (tid < kLinMaxB) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) dzs[tid][cc] = 0.f;
      }
      __syncthreads();

      // ---- the loss and the count by thread 0, db by thread c, the tiles' dz^T x: all in sample order
      if (tid == 0) {
        for (int b = 0; b < srows; ++b) {
          loss_sum += static_cast<double>(lossb[b]);
          correct += corr[b];
        }
      }
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
  }

  // ---- this workgroup's slot: its dW, db, loss sum and count, and nothing else
  float* slot = a.w.plane + static_cast<int64_t>(blockIdx.x) * P;
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d = 16 * (kLinWaves * k + wave) + i0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * q0 + r < C && d < D) slot[(4 * q0 + r) * D + d] = ga[k][r];
  }
  if (tid < C) slot[P0 + tid] = db;
  if (tid == 0) {
    a.w.lc[2 * blockIdx.x] = loss_sum;
    a.w.lc[2 * blockIdx.x + 1] = static_cast<double>(correct);
  }
}

// ---------------------------------------------------------------- a client's slots, its guard and its step
struct CsStep {
  float* rows;
  double* rec;
  CsLayout w;
  double coef[kAdamCoefs];  // Adam: this epoch's row
  double lr_ratio;
  int64_t ld;
  float alpha;
  int P, form, ep, last;  // last: the call's last epoch
};

template <bool ADAM>
__global__ __launch_bounds__(kLinThreads) void client_cosplit_step_kernel(const CsStep a) {
  __shared__ double red[kClientStats][kLinWaves];
  __shared__ float sh_loss;
  __shared__ int sh_correct;
  const int tid = static_cast<int>(threadIdx.x), g = static_cast<int>(blockIdx.x), P = a.P;
  double* st = a.w.state + kCsState * g;
  if (st[0] != 0.0 || st[1] >= 0.0) return;
  const CsEntry e = a.w.tab[g];
  const CsSpan sp = a.w.span[g];
  float* row = a.rows + e.row * a.ld;
  float* last_g = a.w.last_g + static_cast<int64_t>(g) * P;
  const float* plane = a.w.plane + static_cast<int64_t>(sp.first) * P;

  // ---- the loss and the count of this epoch, from before its step: the slots hold them
  if (tid == 0) {
    double sum = 0.0, count = 0.0;
    for (int s = 0; s < sp.n; ++s) {
      sum += a.w.lc[2 * (sp.first + s)];
      count += a.w.lc[2 * (sp.first + s) + 1];
    }
    sh_loss = static_cast<float>(sum / static_cast<double>(e.B));
    sh_correct = static_cast<int>(count);
  }

  // ---- the gradient: slot after slot, parameter tid + 512 (4 j + r) in gv[j][r]
  float gv[kCsStepSlices][4];
#pragma unroll
  for (int j = 0; j < kCsStepSlices; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) gv[j][r] = 0.f;
  // kCsStepAhead slots' loads are in flight before the first of them is added: one workgroup has a client's whole
  // plane to read, and slot by slot it would wait for memory n times.  The adds keep the slot order.
  for (int s0 = 0; s0 < sp.n; s0 += kCsStepAhead) {
    float t[kCsStepAhead][kCsStepSlices][4];
#pragma unroll
    for (int u = 0; u < kCsStepAhead; ++u) {
      const int s = s0 + u < sp.n ? s0 + u : sp.n - 1;  // past the last slot: the last one again, loaded and not added
      const float* slot = plane + static_cast<int64_t>(s) * P;
#pragma unroll
      for (int j = 0; j < kCsStepSlices; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = tid + kLinThreads * (4 * j + r);
          t[u][j][r] = p < P ? slot[p] : 0.f;
        }
    }
#pragma unroll
    for (int u = 0; u < kCsStepAhead; ++u)
#pragma unroll
      for (int j = 0; j < kCsStepSlices; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) gv[j][r] = s0 + u < sp.n ? gv[j][r] + t[u][j][r] : gv[j][r];
  }

  // ---- {NaN count, sum g^2, sum (g - last_g)^2} and norm(last_w)^2; the first epoch's last_grads are its own
  int nans = 0;
  double acc[kClientStats] = {0.0, 0.0, 0.0}, wsq[kClientStats] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < kCsStepSlices; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = tid + kLinThreads * (4 * j + r);
      if (p < P) {
        const float gp = gv[j][r], held = a.ep ? last_g[p] : gp;
        nans += static_cast<int>(gp != gp);
        add_sq(acc[1], static_cast<double>(gp));
        add_sq(acc[2], static_cast<double>(gp - held));
        last_g[p] = gp;
        add_sq(wsq[1], static_cast<double>(row[p]));
      }
    }
  acc[0] = static_cast<double>(nans);
  lin_block_sum(acc, red);
  lin_block_sum(wsq, red);
  const float loss = sh_loss;

  // ---- the :71 guard, the same decision in every thread
  const double n_g = guard_norm<CliOpF32>(acc[1]), n_w = guard_norm<CliOpF32>(wsq[1]);
  if (acc[0] > 0.0 || loss != loss || n_g > guard_bound<CliOpF32>(n_w, a.lr_ratio)) {
    if (tid == 0) {  // the row stays as it stands: the parameters at the trip
      double* rec = a.rec + 8 * e.row;
      rec[0] = static_cast<double>(a.ep);
      rec[1] = static_cast<double>(loss);
      rec[2] = st[5];
      rec[3] = st[4];
      rec[4] = static_cast<double>(sh_correct);
      rec[6] = st[2];
      st[1] = static_cast<double>(a.ep);
    }
    return;
  }

  // ---- the step
  AdamCoef<float> c = {};
  if constexpr (ADAM)
    c = {static_cast<float>(a.coef[0]), static_cast<float>(a.coef[1]), static_cast<float>(a.coef[2]),
         static_cast<float>(a.coef[3]), static_cast<float>(a.coef[4]), static_cast<float>(a.coef[5]),
         static_cast<float>(a.coef[6]), a.form, a.coef[0] != 0.0 ? 1 : 0};
  float* am = ADAM ? a.w.adam + static_cast<int64_t>(g) * 3 * P : nullptr;
  double wst[kClientStats] = {0.0, 0.0, 0.0};
  int wn = 0;
#pragma unroll
  for (int j = 0; j < kCsStepSlices; ++j) {
    float w4[4], m4[4], v4[4], x4[4];
    int live = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = tid + kLinThreads * (4 * j + r);
      const bool on = p < P;
      live += on ? 1 : 0;
      w4[r] = on ? row[p] : 0.f;
      m4[r] = v4[r] = x4[r] = 0.f;
      if constexpr (ADAM) {
        if (on && a.ep) m4[r] = am[p], v4[r] = am[P + p], x4[r] = am[2 * P + p];
      }
    }
    lin_step<ADAM>(w4, gv[j], m4, v4, x4, a.alpha, a.form, c, live, wn, wst[1], wst[2]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = tid + kLinThreads * (4 * j + r);
      if (p < P) {
        row[p] = w4[r];
        if constexpr (ADAM) am[p] = m4[r], am[P + p] = v4[r], am[2 * P + p] = x4[r];
      }
    }
  }
  wst[0] = static_cast<double>(wn);
  lin_block_sum(wst, red);

  // ---- rho / beta (:78-84), and the record when the call ends here
  if (tid == 0) {
    const double last_loss = a.ep ? st[3] : static_cast<double>(loss);
    cli_track<CliOpF32>(st + 4, wst, acc, __builtin_fabs(static_cast<double>(loss) - last_loss));
    st[3] = static_cast<double>(loss);
    st[2] += 1.0;
    if (a.last) {
      double* rec = a.rec + 8 * e.row;
      rec[1] = static_cast<double>(loss);
      rec[2] = st[5];
      rec[3] = st[4];
      rec[4] = static_cast<double>(sh_correct);
      rec[6] = st[2];
    }
  }
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int fedavg_clientcosplit_abi_version(void) { return 1; }

const char* fedavg_clientcosplit_last_error(void) { return g_cs_err.c_str(); }

int64_t fedavg_client_cosplit_workspace_bytes(const int64_t* B, int64_t K, int64_t D, int64_t C,
                                              int64_t slices_per_group, int optimizer) {
  if (!B || K < 1 || K > kCsMaxK || D < 1 || D > kLinMaxD || C < 2 || C > kLinMaxC || slices_per_group < 1 ||
      (optimizer != 0 && optimizer != 1))
    return 0;
  const int64_t R = cs_slice_rows(D);
  int64_t N = 0;
  for (int64_t k = 0; k < K; ++k) {
    if (B[k] < 1 || B[k] > kCsMaxB) return 0;
    N += cs_groups(B[k], R, slices_per_group);
  }
  return cs_workspace(K, N, C * D + C, optimizer == 1);
}

int fedavg_client_cohort_split_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K,
                                   int64_t D, int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                   double lr_ratio, int form, const double* coef, double* rec,
                                   int64_t slices_per_group, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "fedavg_client_cohort_split_f32";
  if (!model || !rows || !clients || !rec || !workspace)
    return cs_error(FEDAVG_EINVAL, "%s: null model, rows, clients, rec or workspace", what);
  if (K < 1 || K > kCsMaxK) return cs_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kCsMaxK);
  if (D < 1 || D > kLinMaxD) return cs_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return cs_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  const int64_t P = C * D + C;
  if (ld < P) return cs_error(FEDAVG_EINVAL, "%s: ld = %lld below P = %lld", what, (long long)ld, (long long)P);
  if (iters < 0 || iters > INT32_MAX) return cs_error(FEDAVG_EINVAL, "%s: negative iteration count", what);
  if (activation != 0 && activation != 1)
    return cs_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return cs_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return cs_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && iters > 0 && !coef) return cs_error(FEDAVG_EINVAL, "%s: null coef", what);
  if (slices_per_group < 1)
    return cs_error(FEDAVG_EINVAL, "%s: slices_per_group = %lld below 1", what, (long long)slices_per_group);
  if (misaligned(model, 4) || misaligned(rows, 4) || misaligned(clients, 8) || misaligned(rec, 8) ||
      (adam && misaligned(coef, 8)) || misaligned(workspace, 8))
    return cs_error(FEDAVG_EALIGN, "%s: model, rows must be 4-B, clients, rec, coef and workspace 8-B aligned", what);

  // ---- the table, read on the host where it lies
  const CsEntry* tab = static_cast<const CsEntry*>(clients);
  const int64_t R = cs_slice_rows(D), q = slices_per_group < kCsMaxB ? slices_per_group : kCsMaxB;
  std::bitset<kCsMaxK> seen;
  bool dma = D % 4 == 0;
  int64_t N = 0;
  for (int64_t g = 0; g < K; ++g) {
    const CsEntry& e = tab[g];
    if (!e.x || !e.y) return cs_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kCsMaxB)
      return cs_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kCsMaxB);
    if (e.row < 0 || e.row >= K)
      return cs_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld outside [0, %lld)", what, (long long)g, (long long)e.row,
                      (long long)K);
    if (seen[e.row]) return cs_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld used twice", what, (long long)g, (long long)e.row);
    seen[e.row] = true;
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return cs_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    dma = dma && !misaligned(e.x, 16);
    N += cs_groups(e.B, R, q);
  }
  if (workspace_bytes < cs_workspace(K, N, P, adam))
    return cs_error(FEDAVG_EINVAL, "%s: workspace of %lld bytes below the %lld of fedavg_client_cosplit_workspace_bytes",
                    what, (long long)workspace_bytes, (long long)cs_workspace(K, N, P, adam));

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return cs_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || !is_device_memory(rows) || !is_device_memory(workspace))
    return cs_error(FEDAVG_EINVAL, "%s: model, rows and workspace must be device memory", what);
  if (!is_device_memory(rec) && !is_pinned_host_memory(rec))
    return cs_error(FEDAVG_EINVAL, "%s: rec must be device or pinned host memory", what);
  if (adam && iters > 0) {
    if (!is_pinned_host_memory(coef)) return cs_error(FEDAVG_EINVAL, "%s: coef is not pinned host memory", what);
    for (int64_t t = 0; t < iters; ++t)
      if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
        return cs_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                        coef[kAdamCoefs * t + 1]);
  }
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return cs_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  const int64_t lds = R * cs_row_floats(D) * 4;
  const auto grad = dma ? client_cosplit_grad_kernel<true> : client_cosplit_grad_kernel<false>;
  const auto step = adam ? client_cosplit_step_kernel<true> : client_cosplit_step_kernel<false>;
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(grad),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return cs_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }

  // ---- 1 + 2 * iters launches, nothing between them but the stream's order
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CsLayout w = cs_layout(workspace, K, N, P, adam);
  const CsSetup su = {model, rows, tab, rec, w, ld, static_cast<int>(K), static_cast<int>(P), static_cast<int>(C),
                      static_cast<int>(R), static_cast<int>(q)};
  hipLaunchKernelGGL(client_cosplit_setup_kernel, dim3(static_cast<unsigned>(K + 1)), dim3(kLinThreads), 0, s, su);
  int rc = launch_status(g_cs_err, what);
  const CsGrad ga = {rows, w, ld, static_cast<int>(D), static_cast<int>(C), static_cast<int>(R), static_cast<int>(q),
                     activation};
  CsStep sa = {rows, rec, w, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lr_ratio, ld,
               static_cast<float>(-lr),  // ATen: rounded once to opmath
               static_cast<int>(P), form, 0, 0};
  for (int64_t ep = 0; ep < iters && rc == FEDAVG_OK; ++ep) {  // a refused launch is not followed by more of them
    hipLaunchKernelGGL(grad, dim3(static_cast<unsigned>(N)), dim3(kLinThreads), static_cast<size_t>(lds), s, ga);
    if (adam)
      for (int j = 0; j < kAdamCoefs; ++j) sa.coef[j] = coef[kAdamCoefs * ep + j];
    sa.ep = static_cast<int>(ep);
    sa.last = ep + 1 == iters ? 1 : 0;
    hipLaunchKernelGGL(step, dim3(static_cast<unsigned>(K)), dim3(kLinThreads), 0, s, sa);
    rc = launch_status(g_cs_err, what);
  }
  return rc;
}

}  // extern "C"
