// fedavg_client_chain.hip -- libfedavg_amd_clientchain.so (include/
// fedavg_amd_clientchain.h): central_train's chain of optimizer steps
// (fedavg_trainer.py:361-371) for a linear softmax model in one launch: ONE
// model, one step on each table entry's whole batch, in table order, `rounds`
// times over, the optimizer state carried from step to step.
//
// The products, the per-sample softmax and the order of every reduction are
// those of the streamed loop (client_stream_core.hpp, whose fetch and whose
// row accessors this unit includes).  What is this unit's own:
//
//   One persistent workgroup, one walk.  The call is one sequence of row groups:
//   entry 0's ceil(B_0 / R) groups, entry 1's, ..., entry K - 1's, then entry
//   0's again.  Group t of the walk lies in LDS buffer t & 1, and the group
//   after it -- of the same entry, of the next entry, or of entry 0 at a
//   round's end -- is requested into the other buffer before group t's forward.
//   So the first rows of the next batch arrive while this batch's last group
//   and its step are formed.  Every batch is read once per round.
//
//   A step at each entry boundary, on registers.  W, the step's gradient and
//   Adam's m, v, vmax are f32x4 per column tile in the layout in which the
//   16x16x4 matrix instruction consumes W and leaves dW.  There is no
//   last_grads array and no statistic: four arrays where the streamed loop
//   holds five.  `model` and `state` are read at entry and written after the
//   call's last step, and at no other time.
//
//   The table and the coefficients through two small LDS rings.  Both may lie
//   in pinned host memory, a PCIe round trip away.  Thread s of the first 64
//   copies step s's entry and coefficient row at entry; from then on, at every
//   32nd step, 32 threads copy the 32 steps that follow the next 32.  A step
//   therefore reads its entry, and the one after it, from LDS.
//
//   All labels first.  The table crosses the link 512 entries at a time into
//   the (still unused) row buffers, wave w checks the labels of entries
//   w, w + 8, ..., and the lowest entry with a label outside [0, C) is
//   reported before anything is trained.
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <climits>

#include "client_stream_core.hpp"
#include "fedavg_amd_clientchain.h"

namespace {

thread_local ErrorState g_ch_err;

int ch_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_ch_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kChMaxK = 4096, kChMaxB = 16384;  // the cohort's ranges
static_assert(static_cast<int64_t>(kChMaxB) * kLinMaxD <= (int64_t{1} << 24), "32-bit indexing");
constexpr int kChRing = 64, kChAhead = kChRing / 2;  // steps whose entry and coefficients lie in LDS; the refill's unit
constexpr int kChLabelChunk = kLinThreads;           // table entries checked per pass of the label check
constexpr int64_t kChMinLds = kChLabelChunk * 32;    // the label check's table chunk lies in the row buffers

// rows per group and floats per LDS row: the stream library's arithmetic (fedavg_client_stream_group_rows)
int64_t ch_row_floats(int64_t D) { return 4 * ((D + 3) / 4) + 4; }
int64_t ch_group_rows(int64_t D) {
  for (int64_t r = kLinMaxB; r > 16; r >>= 1)
    if (2 * r * ch_row_floats(D) * 4 <= kLinResidentBytes) return r;
  return 16;
}

// an entry of the client table, as the header lays it out
struct ChEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t unused;
};
static_assert(sizeof(ChEntry) == 32, "the header's 32-B entry");

struct ChArgs {
  float* model;
  float* state;
  const ChEntry* clients;
  const double* coef;
  double* losses;
  double* rec;
  int64_t step0;
  float alpha;
  int K, D, C, total, act, form, R, two;  // total = rounds * K steps; two: the walk has more than one group
};

// a 64-bit value every lane holds alike, in scalar registers
__device__ __forceinline__ uint64_t ch_uniform(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}

struct ChStep {  // one step's entry as the walk uses it
  const float* x;
  const int64_t* y;
  int B;
};

__device__ __forceinline__ ChStep ch_step_of(const ChEntry& e) {
  return ChStep{reinterpret_cast<const float*>(ch_uniform(reinterpret_cast<uint64_t>(e.x))),
                reinterpret_cast<const int64_t*>(ch_uniform(reinterpret_cast<uint64_t>(e.y))),
                __builtin_amdgcn_readfirstlane(static_cast<int>(e.B))};
}

template <bool ADAM, bool DMA>
__global__ __launch_bounds__(kLinThreads) void client_chain_f32_kernel(const ChArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];  // one or two buffers of R rows of S floats
  __shared__ float part[kLinWaves / 2][kLinMaxB][16];         // the group's partial logits
  __shared__ float dzs[kLinMaxB][16];                         // the group's dz; rows past its end are 0
  __shared__ float lossb[kLinMaxB];
  __shared__ int corr[kLinMaxB];  // lin_sample's; not reported
  __shared__ float bias[16];
  __shared__ ChEntry ring[kChRing];                    // step s's entry in slot s % kChRing
  __shared__ double cring[ADAM ? kChRing : 1][8];      // and its coefficient row
  __shared__ int sh_bad;

  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int K = a.K, D = a.D, C = a.C, R = a.R, D4 = (D + 3) & ~3, S = D4 + 4, total = a.total;

  // ---- every label of every entry, before anything else
  if (tid == 0) sh_bad = INT_MAX;
  {
    ChEntry* tab = reinterpret_cast<ChEntry*>(xs);
    int bad = INT_MAX;
    for (int k0 = 0; k0 < K; k0 += kChLabelChunk) {
      __syncthreads();  // the chunk before this one has been walked
      if (k0 + tid < K) tab[tid] = a.clients[k0 + tid];
      __syncthreads();
      const int n = K - k0 < kChLabelChunk ? K - k0 : kChLabelChunk;
      for (int j = wave; j < n; j += kLinWaves) {
        const ChStep e = ch_step_of(tab[j]);
        for (int b = lane; b < e.B; b += 64) {
          const int64_t y = e.y[b];
          if ((y < 0 || y >= C) && k0 + j < bad) bad = k0 + j;
        }
      }
    }
    if (bad != INT_MAX) atomicMin(&sh_bad, bad);
  }
  __syncthreads();
  if (sh_bad != INT_MAX) {
    if (tid == 0) {
      a.rec[0] = 1.0;
      a.rec[1] = static_cast<double>(sh_bad);
#pragma unroll
      for (int j = 2; j < 8; ++j) a.rec[j] = 0.0;
    }
    return;
  }

  // ---- the first kChRing steps' entries and coefficient rows
  const auto refill = [&](int s) {  // step s < total, by one thread
    ring[s & (kChRing - 1)] = a.clients[s % K];
    if constexpr (ADAM) {
      const double* tc = a.coef + static_cast<int64_t>(kAdamCoefs) * s;
#pragma unroll
      for (int j = 0; j < kAdamCoefs; ++j) cring[s & (kChRing - 1)][j] = tc[j];
    }
  };
  if (tid < kChRing && tid < total) refill(tid);
  __syncthreads();  // the ring is filled, and no wave still reads the label check's table

  // ---- group 0 of step 0 sets out for buffer 0
  ChStep e = ch_step_of(ring[0]);
  str_fetch<DMA>(e.x, xs, 0, e.B < R ? e.B : R, D, D4, S);

  // ---- the parameters and the optimizer's state, in registers for the whole call
  float wv[kLinSlots][4];
  float am[ADAM ? kLinSlots : 1][4], av[ADAM ? kLinSlots : 1][4], ax[ADAM ? kLinSlots : 1][4];
  f32x4 ga[kLinSlots];  // the step's gradient, group by group
  float bw = 0.f, bm = 0.f, bv = 0.f, bx = 0.f;
  const int blive = tid < C ? 1 : 0;  // thread c < C owns b[c], as element 0 of a slice
  const int P0 = C * D, P = P0 + C;
  const bool carried = ADAM && a.step0 > 0;  // m, v, vmax of the steps before this call
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
    ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = i < C && d0 + r < D;
      const int j = on ? i * D + d0 + r : 0;
      const float w = a.model[j];
      wv[k][r] = on ? w : 0.f;
      if constexpr (ADAM) {
        am[k][r] = av[k][r] = ax[k][r] = 0.f;
        if (carried) {
          const float m = a.state[j], v = a.state[P + j], x = a.state[2 * P + j];
          am[k][r] = on ? m : 0.f;
          av[k][r] = on ? v : 0.f;
          ax[k][r] = on ? x : 0.f;
        }
      }
    }
  }
  if (blive) {
    bw = a.model[P0 + tid];
    if (carried) bm = a.state[P0 + tid], bv = a.state[P + P0 + tid], bx = a.state[2 * P + P0 + tid];
  }

  float loss = 0.f;  // thread 0's: the last step's
  int t = 0;         // groups walked: with more than one group in the walk, group t lies in buffer t & 1
  int kk = 0;        // the step's entry
  const int i0 = i, q0 = q;
  for (int s = 0; s < total; ++s) {
    const int i = lin_opaque(i0), q = lin_opaque(q0);
    ChStep nx = e;  // the entry after this one: read a step ahead
    if (s + 1 < total) nx = ch_step_of(ring[(s + 1) & (kChRing - 1)]);
    const int B = e.B, NG = (B + R - 1) / R;
    const float inv_b = 1.0f / static_cast<float>(B);
    if (tid < 16) bias[tid] = bw;
    double loss_sum = 0.0;  // thread 0's, in sample order across the groups
    float db = 0.f;         // thread c's sum of dz[., c], in sample order across the groups

    for (int c = 0; c < NG; ++c, ++t) {
      const int row0 = c * R, rows = B - row0 < R ? B - row0 : R;
      const int MT = (rows + 15) >> 4, KS = (rows + 3) >> 2;
      float* cur = xs + (a.two && (t & 1) ? R * S : 0);
      // ---- S0: this group's rows are in `cur`, and no wave still reads the other buffer
      if constexpr (DMA) str_landed();
      __syncthreads();
      // ---- the ring: at every kChAhead-th step, the kChAhead steps after the next kChAhead.  Every wave has passed
      // the step before this one, so their slots hold steps that are done; they are first read kChAhead - 1 steps
      // (and more barriers) from here.
      if (c == 0 && s > 0 && (s & (kChAhead - 1)) == 0 && tid < kChAhead && s + kChAhead + tid < total)
        refill(s + kChAhead + tid);
      if (a.two) {  // the group after this one: this entry's, the next entry's first, or none after the last step
        float* other = xs + (t & 1 ? 0 : R * S);
        if (c + 1 < NG)
          str_fetch<DMA>(e.x, other, row0 + R, B - row0 - R < R ? B - row0 - R : R, D, D4, S);
        else if (s + 1 < total)
          str_fetch<DMA>(nx.x, other, 0, nx.B < R ? nx.B : R, D, D4, S);
      }
      const LinBatch<true> xb = {cur, e.x, rows, D, D4, S};

      // ---- forward: this wave's part of z = x W^T for the group's row tiles
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

      // ---- one thread per row of the group; the rows past its end leave zero dz
      if (tid < rows) {
        const int64_t y = e.y[row0 + tid];  // checked above; compared, never an index
        lin_sample(part, bias, dzs, tid, static_cast<int>(y), C, a.act, inv_b, lossb[tid], corr[tid]);
      } else if (tid < kLinMaxB) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) dzs[tid][cc] = 0.f;
      }
      __syncthreads();

      // ---- the loss by thread 0, db by thread c, the tiles' x^T dz: all in sample order
      if (tid == 0)
        for (int b = 0; b < rows; ++b) loss_sum += static_cast<double>(lossb[b]);
      if (tid < 16)
        for (int b = 0; b < rows; ++b) db += dzs[b][tid];
#pragma unroll
      for (int k = 0; k < kLinSlots; ++k) {
        const int n0 = 16 * (kLinWaves * k + wave);
        if (n0 < D) {
          for (int ks = 0; ks < KS; ++ks) ga[k] = mfma4(xb.at(4 * ks + q, n0 + i), dzs[4 * ks + q][i], ga[k]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- the entry's gradient is complete: its loss, from before the step, and the step
    if (tid == 0) {
      loss = static_cast<float>(loss_sum / static_cast<double>(B));
      if (kk + 1 == K) a.losses[s / K] = static_cast<double>(loss);  // what :372 logs
    }
    AdamCoef<float> co = {};
    if constexpr (ADAM) {
      const double* tc = cring[s & (kChRing - 1)];
      co = {static_cast<float>(tc[0]), static_cast<float>(tc[1]), static_cast<float>(tc[2]), static_cast<float>(tc[3]),
            static_cast<float>(tc[4]), static_cast<float>(tc[5]), static_cast<float>(tc[6]), a.form, tc[0] != 0.0 ? 1 : 0};
    }
    double wst[2] = {0.0, 0.0};  // the step rules' statistics: not kept here
    int wn = 0;
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int left = D - (16 * (kLinWaves * k + wave) + 4 * q);
      const int live = i < C ? (left < 0 ? 0 : left > 4 ? 4 : left) : 0;
      const float g4[4] = {ga[k][0], ga[k][1], ga[k][2], ga[k][3]};
      lin_step<ADAM>(wv[k], g4, am[ADAM ? k : 0], av[ADAM ? k : 0], ax[ADAM ? k : 0], a.alpha, a.form, co, live, wn,
                     wst[0], wst[1]);
      ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      float w4[4] = {bw, 0.f, 0.f, 0.f}, m4[4] = {bm, 0.f, 0.f, 0.f}, v4[4] = {bv, 0.f, 0.f, 0.f},
            x4[4] = {bx, 0.f, 0.f, 0.f};
      const float g4[4] = {db, 0.f, 0.f, 0.f};
      lin_step<ADAM>(w4, g4, m4, v4, x4, a.alpha, a.form, co, blive, wn, wst[0], wst[1]);
      bw = w4[0], bm = m4[0], bv = v4[0], bx = x4[0];
    }
    e = nx;
    kk = kk + 1 == K ? 0 : kk + 1;
  }

  // ---- what leaves the CU: the model, Adam's state and the record
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i < C && d0 + r < D) {
        const int j = i * D + d0 + r;
        a.model[j] = wv[k][r];
        if constexpr (ADAM) a.state[j] = am[k][r], a.state[P + j] = av[k][r], a.state[2 * P + j] = ax[k][r];
      }
  }
  if (blive) {
    a.model[P0 + tid] = bw;
    if constexpr (ADAM) a.state[P0 + tid] = bm, a.state[P + P0 + tid] = bv, a.state[2 * P + P0 + tid] = bx;
  }
  if (tid == 0) {
    a.rec[0] = 0.0;
    a.rec[1] = -1.0;
    a.rec[2] = static_cast<double>(total);
    a.rec[3] = static_cast<double>(loss);
#pragma unroll
    for (int j = 4; j < 8; ++j) a.rec[j] = 0.0;
  }
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

template <bool ADAM, bool DMA>
int ch_launch(const char* what, const ChArgs& a, int64_t lds, hipStream_t s) {
  const auto kernel = client_chain_f32_kernel<ADAM, DMA>;
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return ch_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL(kernel, dim3(1), dim3(kLinThreads), static_cast<size_t>(lds), s, a);
  return launch_status(g_ch_err, what);
}

}  // namespace

extern "C" {

int fedavg_clientchain_abi_version(void) { return 1; }

const char* fedavg_clientchain_last_error(void) { return g_ch_err.c_str(); }

void fedavg_client_chain_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c) {
  if (max_k) *max_k = kChMaxK;
  if (max_b) *max_b = kChMaxB;
  if (max_d) *max_d = kLinMaxD;
  if (max_c) *max_c = kLinMaxC;
}

int fedavg_client_chain_f32(float* model, float* state, const void* clients, int64_t K, int64_t D, int64_t C,
                            int64_t rounds, int64_t step0, int activation, int optimizer, double lr, int form,
                            const double* coef, double* losses, double* rec, void* stream) {
  const char* what = "fedavg_client_chain_f32";
  if (!model || !clients || !losses || !rec) return ch_error(FEDAVG_EINVAL, "%s: null model, clients, losses or rec", what);
  if (K < 1 || K > kChMaxK) return ch_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kChMaxK);
  if (D < 1 || D > kLinMaxD) return ch_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return ch_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  if (rounds < 1 || rounds > INT32_MAX / K)
    return ch_error(FEDAVG_EINVAL, "%s: rounds = %lld outside [1, %lld]", what, (long long)rounds,
                    (long long)(INT32_MAX / K));
  if (step0 < 0) return ch_error(FEDAVG_EINVAL, "%s: step0 = %lld is negative", what, (long long)step0);
  if (activation != 0 && activation != 1)
    return ch_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return ch_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return ch_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && !state) return ch_error(FEDAVG_EINVAL, "%s: null state", what);
  if (adam && !coef) return ch_error(FEDAVG_EINVAL, "%s: null coef", what);
  if (misaligned(model, 4) || (adam && misaligned(state, 4)) || misaligned(clients, 8) || misaligned(losses, 8) ||
      misaligned(rec, 8) || (adam && misaligned(coef, 8)))
    return ch_error(FEDAVG_EALIGN, "%s: model, state must be 4-B, clients, losses, rec and coef 8-B aligned", what);

  // ---- the table, read on the host where it lies, in its own order
  const ChEntry* tab = static_cast<const ChEntry*>(clients);
  const int64_t R = ch_group_rows(D);
  bool dma = D % 4 == 0;
  for (int64_t g = 0; g < K; ++g) {
    const ChEntry& e = tab[g];
    if (!e.x || !e.y) return ch_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kChMaxB)
      return ch_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kChMaxB);
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return ch_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    dma = dma && !misaligned(e.x, 16);
  }
  const bool two = K > 1 || tab[0].B > R;  // else the one batch is loaded once and stays

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return ch_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || (adam && !is_device_memory(state)))
    return ch_error(FEDAVG_EINVAL, "%s: model and state must be device memory", what);
  for (const double* p : {losses, rec})
    if (!is_device_memory(p) && !is_pinned_host_memory(p))
      return ch_error(FEDAVG_EINVAL, "%s: losses and rec must be device or pinned host memory", what);
  if (adam) {
    if (is_pinned_host_memory(coef)) {
      for (int64_t t = 0; t < rounds * K; ++t)
        if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
          return ch_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                          coef[kAdamCoefs * t + 1]);
    } else if (!is_device_memory(coef)) {
      return ch_error(FEDAVG_EINVAL, "%s: coef must be device or pinned host memory", what);
    }
  }
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return ch_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  const ChArgs a = {model, adam ? state : nullptr, tab, coef, losses, rec, step0,
                    static_cast<float>(-lr),  // ATen: rounded once to opmath
                    static_cast<int>(K), static_cast<int>(D), static_cast<int>(C), static_cast<int>(rounds * K),
                    activation, form, static_cast<int>(R), two ? 1 : 0};
  const int64_t rows_lds = (two ? 2 : 1) * R * ch_row_floats(D) * 4;
  const int64_t lds = rows_lds < kChMinLds ? kChMinLds : rows_lds;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dma) return adam ? ch_launch<true, true>(what, a, lds, s) : ch_launch<false, true>(what, a, lds, s);
  return adam ? ch_launch<true, false>(what, a, lds, s) : ch_launch<false, false>(what, a, lds, s);
}

}  // extern "C"
