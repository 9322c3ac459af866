// fedavg_client_wide.hip -- libfedavg_amd_clientwide.so (include/fedavg_amd_clientwide.h): the local loops of ALL the
// linear clients of a round (fedavg_trainer.py:172-199) for models of up to 128 classes and 4096 columns.  The other
// linear kernels feed W to the matrix instruction as ONE class tile and keep whole rows of x in LDS (or W, its
// gradient and Adam's state in registers); here everything is tiled over classes and over columns, and no workgroup
// holds a full row of x or a full W.  A call is a setup launch and four launches per local iteration, in stream
// order, with nothing else between them:
//
//   setup    : as fedavg_client_cosplit.hip's.  K + 1 workgroups: labels, rows, state blocks, records; the group
//              table.  A slice is R = 64 rows; client k has G_k = ceil(B_k / 64) slices and ceil(G_k / q) workgroups.
//   gradient : one workgroup of 512 threads per group of q slices.  x moves in UNITS of 64 rows x 128 columns through
//              two LDS buffers (rows of 132 floats: the A operand's 16-B reads of sixteen rows fall on different
//              banks).  With D % 4 == 0 and every x 16-B aligned a unit goes from global memory straight into LDS,
//              one row of 512 B per wave instruction (lanes 0 .. 31; the instruction writes lane after lane, so it
//              cannot skip the four pad floats and a row is all it covers), else it is staged through registers.
//              Either way every float of the 64 x 128 is written: what lies past the batch or past D is zero.  The
//              next unit of the walk is requested before the current one is consumed.
//                forward  (slice, then panel): product (row tile mt, class tile ct), p = mt + 4 ct, belongs to wave
//                  p % 8 for the whole of D: wave w has row tile w & 3 and class tiles (w >> 2) + 2 j, so its A
//                  operand is read once for up to four products.  W comes from the client's row (L2) into the B
//                  operand.  With fewer than two class tiles waves 4 .. 7 have no product; that is accepted.
//                  After the last panel z goes to the dz store, rows of 16 CT + 1 floats.
//                per-sample (one thread per row, C logits in class order): bias, sigmoid, log-softmax, loss term,
//                  argmax, dz in place.  Thread 0 adds the loss terms and counts, thread c the column c of dz, both
//                  in sample order.
//                backward (panel, then slice): wave w owns column block w of the panel for every class tile; its
//                  dW tiles accumulate dz^T x over the group's slices in slice order and are written once to the
//                  workgroup's slot.  No dW register outlives a panel.
//   sum      : grid (chunks of 8192 parameters, clients).  The client's slots in slot order, four slots' loads in
//              flight, into g[ep & 1]; per chunk {NaN count, sum g^2, sum (g - last_g)^2, sum w^2}.
//   step     : the same grid.  Thread 0 of every workgroup adds its client's loss sums in slot order and its chunk
//              partials in chunk order (cw_verdict): every workgroup of a client reaches the same verdict on the :71
//              guard.  Then lin_step on the chunk of the row, and the partial of sum (w' - w)^2.
//   track    : one workgroup per client: cw_verdict again, the trip or rho / beta, the record.
//
// last_grads is g[(ep & 1) ^ 1]: the two gradient blocks change roles every epoch.
//
// Workspace, for N slots, P parameters and NC = ceil(P / 8192) chunks: tab [K] 32 B, state [K] 64 B, span [K] 8 B,
// groups [N] 8 B, lc [N, 2] fp64, part [K, NC, 4] fp64, spart [K, NC] fp64, g [2, K, P], Adam's [K, 3, P] (Adam calls
// only), plane [N, P].
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <bitset>

#include "client_stream_core.hpp"
#include "fedavg_amd_clientwide.h"

namespace {

thread_local ErrorState g_cw_err;

int cw_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_cw_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kCwMaxK = 4096, kCwMaxB = 16384, kCwMaxD = 4096, kCwMaxC = 128;
constexpr int64_t kCwMaxP = static_cast<int64_t>(kCwMaxC) * (kCwMaxD + 1);
static_assert(static_cast<int64_t>(kCwMaxB) * kCwMaxD <= (int64_t{1} << 26), "32-bit indexing of a batch");
constexpr int kCwR = 64;                 // rows of a slice: four row tiles
constexpr int kCwDP = 128;               // columns of a panel
constexpr int kCwS = kCwDP + 4;          // floats of a unit's row in LDS
constexpr int kCwUnit = kCwR * kCwS;     // floats of a unit buffer
constexpr int kCwMaxCT = kCwMaxC / 16;   // class tiles
constexpr int kCwMaxQ = 15;              // the largest slices_per_group (at one class tile)
constexpr int kCwChunk = 8192;           // parameters of a chunk of the sum and step launches
constexpr int kCwAhead = 4;              // the sum launch: slots whose loads are in flight together
constexpr int kCwState = 8;              // doubles of a client's state block
constexpr int kCwScanChunk = kLinThreads;
static_assert(kCwChunk == 16 * kLinThreads && kLinWaves == 8 && kCwDP == 16 * kLinWaves, "the kernels' dealing");

// the dz store: a row of 16 CT + 1 floats per sample (the odd stride: the rows of the per-sample pass on different banks)
int64_t cw_tiles(int64_t C) { return (C + 15) / 16; }
int64_t cw_dz_bytes(int64_t C) { return kCwR * (16 * cw_tiles(C) + 1) * 4; }
int64_t cw_max_slices(int64_t C) {
  if (C < 2 || C > kCwMaxC) return 0;
  const int64_t q = (kLinResidentBytes - 2 * kCwUnit * 4) / cw_dz_bytes(C);
  return q > kCwMaxQ ? kCwMaxQ : q;
}
int64_t cw_groups(int64_t B, int64_t q) { return ((B + kCwR - 1) / kCwR + q - 1) / q; }
int64_t cw_chunks(int64_t P) { return (P + kCwChunk - 1) / kCwChunk; }
int64_t cw_workspace(int64_t K, int64_t N, int64_t P, bool adam) {
  return 104 * K + 24 * N + 40 * K * cw_chunks(P) + 4 * P * (N + K * (adam ? 5 : 2));
}

// an entry of the client table, as the cohort's header lays it out
struct CwEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t row;
};
static_assert(sizeof(CwEntry) == 32, "the header's 32-B entry");

struct CwSpan {
  int first, n;  // a client's slots of the plane
};
struct CwGroup {
  int entry, slice0;  // a slot's client and the first slice of its workgroup
};

struct CwLayout {
  CwEntry* tab;
  double* state;
  CwSpan* span;
  CwGroup* groups;
  double* lc;
  double* part;
  double* spart;
  float* g;
  float* adam;
  float* plane;
};

CwLayout cw_layout(void* workspace, int64_t K, int64_t N, int64_t P, bool adam) {
  char* p = static_cast<char*>(workspace);
  const int64_t NC = cw_chunks(P);
  CwLayout w;
  w.tab = reinterpret_cast<CwEntry*>(p), p += 32 * K;
  w.state = reinterpret_cast<double*>(p), p += 8 * kCwState * K;
  w.span = reinterpret_cast<CwSpan*>(p), p += 8 * K;
  w.groups = reinterpret_cast<CwGroup*>(p), p += 8 * N;
  w.lc = reinterpret_cast<double*>(p), p += 16 * N;
  w.part = reinterpret_cast<double*>(p), p += 32 * K * NC;
  w.spart = reinterpret_cast<double*>(p), p += 8 * K * NC;
  w.g = reinterpret_cast<float*>(p), p += 8 * P * K;
  w.adam = reinterpret_cast<float*>(p), p += adam ? 12 * P * K : 0;
  w.plane = reinterpret_cast<float*>(p);
  return w;
}

// ---------------------------------------------------------------- labels, rows, state, records; the group table
struct CwSetup {
  const float* model;
  float* rows;
  const CwEntry* clients;
  double* rec;
  CwLayout w;
  int64_t ld;
  int K, P, C, q;
};

__global__ __launch_bounds__(kLinThreads) void client_wide_setup_kernel(const CwSetup a) {
  __shared__ int ns[kCwScanChunk];
  __shared__ int sh_flag;
  const int tid = static_cast<int>(threadIdx.x), g = static_cast<int>(blockIdx.x);
  if (g < a.K) {
    const CwEntry e = a.clients[g];  // uniform: the workgroup's own client
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
      double* st = a.w.state + kCwState * g;
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
  for (int k0 = 0; k0 < a.K; k0 += kCwScanChunk) {
    __syncthreads();  // the chunk before this one has been added up
    const int k = k0 + tid;
    int n = 0;
    if (k < a.K) {
      const int B = static_cast<int>(a.clients[k].B);
      n = ((B + kCwR - 1) / kCwR + a.q - 1) / a.q;
    }
    ns[tid] = n;
    __syncthreads();
    int first = base;
    for (int t = 0; t < kCwScanChunk; ++t) {
      if (t == tid) first = base;
      base += ns[t];
    }
    if (k < a.K) {
      a.w.span[k] = CwSpan{first, n};
      for (int j = 0; j < n; ++j) a.w.groups[first + j] = CwGroup{k, j * a.q};
    }
  }
}

// ---------------------------------------------------------------- one workgroup's partial gradient
struct CwGrad {
  const float* rows;
  CwLayout w;
  int64_t ld;
  int D, C, q, act;
};

// Rows [row0, row0 + rows) x columns [c0, c0 + 128) of x into `buf`, rows of kCwS floats; every float of the 64 x 128
// is written, with 0 past the batch or past D.  DMA (D % 4 == 0, x 16-B aligned): a wave instruction carries one row,
// 16 B per lane of lanes 0 .. 31, and nothing is held in registers; the caller waits with str_landed().
template <bool DMA>
__device__ __forceinline__ void cw_fetch(const float* x, float* buf, int row0, int rows, int c0, int D) {
  const int tid = static_cast<int>(threadIdx.x);
  if constexpr (DMA) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, col = c0 + 4 * lane;
    if (lane < kCwDP / 4) {
      for (int rl = wave; rl < kCwR; rl += kLinWaves) {
        if (rl < rows && col < D)  // D % 4 == 0: the lane's 16 B lie inside the row
          __builtin_amdgcn_global_load_lds((str_global_ptr)(x + (row0 + rl) * D + col), (str_lds_ptr)(buf + rl * kCwS),
                                           16, 0, 0);
        else
          *reinterpret_cast<f32x4*>(buf + rl * kCwS + 4 * lane) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  } else {
    for (int idx = tid; idx < kCwR * (kCwDP / 4); idx += kLinThreads) {
      const int rl = idx >> 5, col = c0 + 4 * (idx & 31);
      const float* src = x + (rl < rows ? row0 + rl : 0) * D;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = rl < rows && col + r < D;
        const float e = src[on ? col + r : 0];
        v[r] = on ? e : 0.f;
      }
      *reinterpret_cast<f32x4*>(buf + rl * kCwS + 4 * (idx & 31)) = v;
    }
  }
}

// One sample, by its thread: lin_sample's walk over C logits in class order (its loss term and argmax; softmax as a
// quotient, below), in place: z[0 .. C) becomes dz, z[C .. CW) zero.
__device__ __forceinline__ void cw_sample(float* z, const float* bias, int y, int C, int CW, int sigmoid, float inv_b,
                                          float& loss, int& correct) {
  float mx = 0.f;
  int arg = 0;
  for (int c = 0; c < C; ++c) {
    const float zc = z[c] + bias[c];
    const float a = sigmoid ? 1.0f / (1.0f + __builtin_expf(-zc)) : zc;
    z[c] = a;
    if (c == 0) {
      mx = a;
    } else if (a > mx) {  // strict: a tie keeps the first index
      mx = a;
      arg = c;
    }
  }
  float se = 0.f;
  for (int c = 0; c < C; ++c) se += __builtin_expf(z[c] - mx);
  const float lse = __builtin_logf(se);
  float ly = 0.f;
  for (int c = 0; c < C; ++c) {
    const float a = z[c];
    if (c == y) ly = (a - mx) - lse;  // log_softmax
    // softmax as the quotient, not as exp(log_softmax): at up to 128 classes log_softmax is several units large and
    // its rounding is a common factor of every p of the row (2^-22 at 4), which beta's difference of two epochs'
    // gradients amplifies; the quotient's common factor is se's rounding alone
    const float p = __builtin_expf(a - mx) / se;
    const float da = p * inv_b - (c == y ? inv_b : 0.f);
    z[c] = sigmoid ? da * a * (1.0f - a) : da;
  }
  for (int c = C; c < CW; ++c) z[c] = 0.f;
  loss = -ly;
  correct = arg == y ? 1 : 0;
}

template <bool DMA>
__global__ __launch_bounds__(kLinThreads) void client_wide_grad_kernel(const CwGrad a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // two unit buffers, then the dz store
  __shared__ float lossb[kCwMaxQ * kCwR];
  __shared__ int corr[kCwMaxQ * kCwR];
  __shared__ float bias[kCwMaxC];

  const CwGroup gr = a.w.groups[blockIdx.x];
  const double* st = a.w.state + kCwState * gr.entry;
  if (st[0] != 0.0 || st[1] >= 0.0) return;  // a bad label or a tripped guard: nothing is read or written
  const CwEntry e = a.w.tab[gr.entry];

  const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int B = static_cast<int>(e.B), D = a.D, C = a.C, P0 = C * D;
  const int CT = (C + 15) >> 4, ZS = 16 * CT + 1, NP = (D + kCwDP - 1) / kCwDP;
  const int G = (B + kCwR - 1) / kCwR, nsl = (gr.slice0 + a.q < G ? gr.slice0 + a.q : G) - gr.slice0;
  const int brow0 = gr.slice0 * kCwR, brows = B - brow0 < nsl * kCwR ? B - brow0 : nsl * kCwR;  // the group's rows
  const float* model = a.rows + e.row * a.ld;
  float* zs = lds + 2 * kCwUnit;

  // unit t of the walk: the forward's (slice t / NP, panel t % NP), then the backward's (panel, slice)
  const int TF = nsl * NP, T = 2 * TF;
  const auto fetch = [&](int t) {
    const int sl = t < TF ? t / NP : (t - TF) % nsl, pn = t < TF ? t % NP : (t - TF) / nsl;
    const int row0 = brow0 + sl * kCwR;
    cw_fetch<DMA>(e.x, lds + (t & 1) * kCwUnit, row0, B - row0 < kCwR ? B - row0 : kCwR, pn * kCwDP, D);
  };
  fetch(0);
  if (tid < kCwMaxC) {
    const float bw = model[P0 + (tid < C ? tid : 0)];
    bias[tid] = tid < C ? bw : 0.f;
  }

  // ---- forward: this wave's products of z = x W^T, each over the whole of D
  const int mt = wave & 3;
  f32x4 z[4];
  for (int t = 0; t < TF; ++t) {
    const int sl = t / NP, pn = t - sl * NP, c0 = pn * kCwDP;
    const int srows = brows - sl * kCwR < kCwR ? brows - sl * kCwR : kCwR;
    // ---- unit t is in its buffer, and no wave still reads the other one
    if constexpr (DMA) str_landed();
    __syncthreads();
    fetch(t + 1);  // t + 1 < T: the backward follows
    const float* xs = lds + (t & 1) * kCwUnit;
    if (pn == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j) z[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (16 * mt < srows && (wave >> 2) < CT) {
#pragma unroll
      for (int cb = 0; cb < kCwDP / 16; ++cb) {
        const int d0 = c0 + 16 * cb + 4 * q;
        if (c0 + 16 * cb < D) {
          const f32x4 xa = *reinterpret_cast<const f32x4*>(xs + (16 * mt + i) * kCwS + 16 * cb + 4 * q);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int cls = 16 * ((wave >> 2) + 2 * j) + i;
            if ((wave >> 2) + 2 * j < CT) {
              float wv[4];
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const bool on = cls < C && d0 + r < D;
                const float w = model[on ? cls * D + d0 + r : 0];
                wv[r] = on ? w : 0.f;
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) z[j] = mfma4(xa[r], wv[r], z[j]);
            }
          }
        }
      }
    }
    if (pn == NP - 1) {  // the slice's logits: row 16 mt + 4 q + r, class 16 ct + i
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ct = (wave >> 2) + 2 * j;
        if (ct < CT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) zs[(sl * kCwR + 16 * mt + 4 * q + r) * ZS + 16 * ct + i] = z[j][r];
        }
      }
    }
  }
  __syncthreads();  // the group's logits and the bias are in LDS

  // ---- one thread per row of the group; the rows past the batch's end leave zero dz
  const float inv_b = 1.0f / static_cast<float>(B);
  for (int rr = tid; rr < nsl * kCwR; rr += kLinThreads) {
    if (rr < brows) {
      const int64_t y = e.y[brow0 + rr];  // checked by the setup launch; compared, never an index
      cw_sample(zs + rr * ZS, bias, static_cast<int>(y), C, 16 * CT, a.act, inv_b, lossb[rr], corr[rr]);
    } else {
      for (int c = 0; c < 16 * CT; ++c) zs[rr * ZS + c] = 0.f;
    }
  }
  __syncthreads();

  // ---- the loss and the count by thread 0, db by thread c: in sample order
  float* slot = a.w.plane + static_cast<int64_t>(blockIdx.x) * (P0 + C);
  if (tid == 0) {
    double loss_sum = 0.0;
    int correct = 0;
    for (int b = 0; b < brows; ++b) {
      loss_sum += static_cast<double>(lossb[b]);
      correct += corr[b];
    }
    a.w.lc[2 * blockIdx.x] = loss_sum;
    a.w.lc[2 * blockIdx.x + 1] = static_cast<double>(correct);
  }
  if (tid < C) {
    float db = 0.f;
    for (int b = 0; b < brows; ++b) db += zs[b * ZS + tid];
    slot[P0 + tid] = db;
  }

  // ---- backward: column block `wave` of every panel, all class tiles; ga[ct][r] is class 16 ct + 4 q + r, column
  // c0 + 16 wave + i
  f32x4 ga[kCwMaxCT];
  for (int t = TF; t < T; ++t) {
    const int pn = (t - TF) / nsl, sl = (t - TF) - pn * nsl, c0 = pn * kCwDP;
    const int srows = brows - sl * kCwR < kCwR ? brows - sl * kCwR : kCwR, KS = (srows + 3) >> 2;
    if constexpr (DMA) str_landed();
    __syncthreads();
    if (t + 1 < T) fetch(t + 1);
    const float* xs = lds + (t & 1) * kCwUnit;
    const float* dz = zs + sl * kCwR * ZS;
    if (sl == 0) {
#pragma unroll
      for (int ct = 0; ct < kCwMaxCT; ++ct) ga[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bool live = c0 + 16 * wave < D;
    if (live) {
      for (int ks = 0; ks < KS; ++ks) {
        const float xv = xs[(4 * ks + q) * kCwS + 16 * wave + i];
#pragma unroll
        for (int ct = 0; ct < kCwMaxCT; ++ct)
          if (ct < CT) ga[ct] = mfma4(dz[(4 * ks + q) * ZS + 16 * ct + i], xv, ga[ct]);
      }
    }
    if (sl == nsl - 1 && live) {  // the panel's tiles, once, to this workgroup's slot
      const int d = c0 + 16 * wave + i;
#pragma unroll
      for (int ct = 0; ct < kCwMaxCT; ++ct) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int cls = 16 * ct + 4 * q + r;
          if (ct < CT && cls < C && d < D) slot[cls * D + d] = ga[ct][r];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- a client's slots into its gradient, chunk by chunk
struct CwSum {
  const float* rows;
  CwLayout w;
  int64_t ld;
  int K, P, NC, ep;
};

__global__ __launch_bounds__(kLinThreads) void client_wide_sum_kernel(const CwSum a) {
  __shared__ double red[kClientStats][kLinWaves];
  const int tid = static_cast<int>(threadIdx.x), ch = static_cast<int>(blockIdx.x), g = static_cast<int>(blockIdx.y);
  const double* st = a.w.state + kCwState * g;
  if (st[0] != 0.0 || st[1] >= 0.0) return;
  const CwEntry e = a.w.tab[g];
  const CwSpan sp = a.w.span[g];
  const int P = a.P, p0 = ch * kCwChunk + tid;
  const float* row = a.rows + e.row * a.ld;
  float* gcur = a.w.g + (static_cast<int64_t>(a.ep & 1) * a.K + g) * P;
  const float* glast = a.w.g + (static_cast<int64_t>((a.ep & 1) ^ 1) * a.K + g) * P;
  const float* plane = a.w.plane + static_cast<int64_t>(sp.first) * P;

  // ---- parameter p0 + 512 j in gv[j]; kCwAhead slots' loads are in flight before the first of them is added, and the
  // adds keep the slot order
  float gv[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) gv[j] = 0.f;
  for (int s0 = 0; s0 < sp.n; s0 += kCwAhead) {
    float t[kCwAhead][16];
#pragma unroll
    for (int u = 0; u < kCwAhead; ++u) {
      const int s = s0 + u < sp.n ? s0 + u : sp.n - 1;  // past the last slot: the last one again, loaded and not added
      const float* slot = plane + static_cast<int64_t>(s) * P;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int p = p0 + kLinThreads * j;
        t[u][j] = p < P ? slot[p] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < kCwAhead; ++u)
#pragma unroll
      for (int j = 0; j < 16; ++j) gv[j] = s0 + u < sp.n ? gv[j] + t[u][j] : gv[j];
  }

  // ---- {NaN count, sum g^2, sum (g - last_g)^2} and sum w^2; the first epoch's last_grads are its own
  int nans = 0;
  double acc[kClientStats] = {0.0, 0.0, 0.0}, wsq[kClientStats] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int p = p0 + kLinThreads * j;
    if (p < P) {
      const float gp = gv[j], held = a.ep ? glast[p] : gp;
      nans += static_cast<int>(gp != gp);
      add_sq(acc[1], static_cast<double>(gp));
      add_sq(acc[2], static_cast<double>(gp - held));
      gcur[p] = gp;
      add_sq(wsq[1], static_cast<double>(row[p]));
    }
  }
  acc[0] = static_cast<double>(nans);
  lin_block_sum(acc, red);
  lin_block_sum(wsq, red);
  if (tid == 0) {
    double* part = a.w.part + 4 * (static_cast<int64_t>(g) * a.NC + ch);
    part[0] = acc[0], part[1] = acc[1], part[2] = acc[2], part[3] = wsq[1];
  }
}

// ---------------------------------------------------------------- the guard's verdict, the step, the track
// What one thread learns of client g's epoch from the slots' loss sums (slot order) and the chunks' partials (chunk
// order): the step launch's workgroups and the track launch run the same statements on the same values.
struct CwVerdict {
  double acc[kClientStats];
  float loss;
  int correct;
  bool trip;
};

__device__ __forceinline__ CwVerdict cw_verdict(const CwLayout& w, int g, const CwSpan sp, int64_t B, int NC,
                                                double lr_ratio) {
  CwVerdict v;
  double sum = 0.0, count = 0.0;
  for (int s = 0; s < sp.n; ++s) {
    sum += w.lc[2 * (sp.first + s)];
    count += w.lc[2 * (sp.first + s) + 1];
  }
  v.loss = static_cast<float>(sum / static_cast<double>(B));
  v.correct = static_cast<int>(count);
  double wsq = 0.0;
  v.acc[0] = v.acc[1] = v.acc[2] = 0.0;
  for (int c = 0; c < NC; ++c) {
    const double* part = w.part + 4 * (static_cast<int64_t>(g) * NC + c);
    v.acc[0] += part[0], v.acc[1] += part[1], v.acc[2] += part[2], wsq += part[3];
  }
  const double n_g = guard_norm<CliOpF32>(v.acc[1]), n_w = guard_norm<CliOpF32>(wsq);
  v.trip = v.acc[0] > 0.0 || v.loss != v.loss || n_g > guard_bound<CliOpF32>(n_w, lr_ratio);
  return v;
}

struct CwStep {
  float* rows;
  double* rec;
  CwLayout w;
  double coef[kAdamCoefs];  // Adam: this epoch's row
  double lr_ratio;
  int64_t ld;
  float alpha;
  int K, P, NC, form, ep, last;  // last: the call's last epoch
};

template <bool ADAM>
__global__ __launch_bounds__(kLinThreads) void client_wide_step_kernel(const CwStep a) {
  __shared__ double red[kClientStats][kLinWaves];
  __shared__ int sh_trip;
  const int tid = static_cast<int>(threadIdx.x), ch = static_cast<int>(blockIdx.x), g = static_cast<int>(blockIdx.y);
  const double* st = a.w.state + kCwState * g;
  if (st[0] != 0.0 || st[1] >= 0.0) return;
  const CwEntry e = a.w.tab[g];
  if (tid == 0) sh_trip = cw_verdict(a.w, g, a.w.span[g], e.B, a.NC, a.lr_ratio).trip ? 1 : 0;
  __syncthreads();
  if (sh_trip) return;  // the row stays as it stands: the parameters at the trip

  const int P = a.P, p0 = ch * kCwChunk + tid;
  float* row = a.rows + e.row * a.ld;
  const float* gcur = a.w.g + (static_cast<int64_t>(a.ep & 1) * a.K + g) * P;
  AdamCoef<float> c = {};
  if constexpr (ADAM)
    c = {static_cast<float>(a.coef[0]), static_cast<float>(a.coef[1]), static_cast<float>(a.coef[2]),
         static_cast<float>(a.coef[3]), static_cast<float>(a.coef[4]), static_cast<float>(a.coef[5]),
         static_cast<float>(a.coef[6]), a.form, a.coef[0] != 0.0 ? 1 : 0};
  float* am = ADAM ? a.w.adam + static_cast<int64_t>(g) * 3 * P : nullptr;
  double wst[kClientStats] = {0.0, 0.0, 0.0};
  int wn = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float w4[4], g4[4], m4[4], v4[4], x4[4];
    int live = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + kLinThreads * (4 * j + r);
      const bool on = p < P;
      live += on ? 1 : 0;
      w4[r] = on ? row[p] : 0.f;
      g4[r] = on ? gcur[p] : 0.f;
      m4[r] = v4[r] = x4[r] = 0.f;
      if constexpr (ADAM) {
        if (on && a.ep) m4[r] = am[p], v4[r] = am[P + p], x4[r] = am[2 * static_cast<int64_t>(P) + p];
      }
    }
    lin_step<ADAM>(w4, g4, m4, v4, x4, a.alpha, a.form, c, live, wn, wst[1], wst[2]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = p0 + kLinThreads * (4 * j + r);
      if (p < P) {
        row[p] = w4[r];
        if constexpr (ADAM) am[p] = m4[r], am[P + p] = v4[r], am[2 * static_cast<int64_t>(P) + p] = x4[r];
      }
    }
  }
  wst[0] = static_cast<double>(wn);
  lin_block_sum(wst, red);
  if (tid == 0) a.w.spart[static_cast<int64_t>(g) * a.NC + ch] = wst[2];
}

__global__ __launch_bounds__(64) void client_wide_track_kernel(const CwStep a) {
  const int g = static_cast<int>(blockIdx.x);
  double* st = a.w.state + kCwState * g;
  if (threadIdx.x != 0 || st[0] != 0.0 || st[1] >= 0.0) return;
  const CwEntry e = a.w.tab[g];
  const CwVerdict v = cw_verdict(a.w, g, a.w.span[g], e.B, a.NC, a.lr_ratio);
  double* rec = a.rec + 8 * e.row;
  if (v.trip) {
    rec[0] = static_cast<double>(a.ep);
    rec[1] = static_cast<double>(v.loss);
    rec[2] = st[5];
    rec[3] = st[4];
    rec[4] = static_cast<double>(v.correct);
    rec[6] = st[2];
    st[1] = static_cast<double>(a.ep);
    return;
  }
  double wst[kClientStats] = {0.0, 0.0, 0.0};
  for (int c = 0; c < a.NC; ++c) wst[2] += a.w.spart[static_cast<int64_t>(g) * a.NC + c];
  // ---- rho / beta (:78-84), and the record when the call ends here
  const double last_loss = a.ep ? st[3] : static_cast<double>(v.loss);
  cli_track<CliOpF32>(st + 4, wst, v.acc, __builtin_fabs(static_cast<double>(v.loss) - last_loss));
  st[3] = static_cast<double>(v.loss);
  st[2] += 1.0;
  if (a.last) {
    rec[1] = static_cast<double>(v.loss);
    rec[2] = st[5];
    rec[3] = st[4];
    rec[4] = static_cast<double>(v.correct);
    rec[6] = st[2];
  }
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

extern "C" {

int fedavg_clientwide_abi_version(void) { return 1; }

const char* fedavg_clientwide_last_error(void) { return g_cw_err.c_str(); }

void fedavg_client_wide_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c, int64_t* max_p) {
  if (max_k) *max_k = kCwMaxK;
  if (max_b) *max_b = kCwMaxB;
  if (max_d) *max_d = kCwMaxD;
  if (max_c) *max_c = kCwMaxC;
  if (max_p) *max_p = kCwMaxP;
}

int64_t fedavg_client_wide_slice_rows(void) { return kCwR; }

int64_t fedavg_client_wide_max_slices(int64_t C) { return cw_max_slices(C); }

int64_t fedavg_client_wide_workspace_bytes(const int64_t* B, int64_t K, int64_t D, int64_t C, int64_t slices_per_group,
                                           int optimizer) {
  if (!B || K < 1 || K > kCwMaxK || D < 1 || D > kCwMaxD || C < 2 || C > kCwMaxC || slices_per_group < 1 ||
      slices_per_group > cw_max_slices(C) || (optimizer != 0 && optimizer != 1))
    return 0;
  int64_t N = 0;
  for (int64_t k = 0; k < K; ++k) {
    if (B[k] < 1 || B[k] > kCwMaxB) return 0;
    N += cw_groups(B[k], slices_per_group);
  }
  return cw_workspace(K, N, C * D + C, optimizer == 1);
}

int fedavg_client_cohort_wide_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K, int64_t D,
                                  int64_t C, int64_t iters, int activation, int optimizer, double lr, double lr_ratio,
                                  int form, const double* coef, double* rec, int64_t slices_per_group, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  const char* what = "fedavg_client_cohort_wide_f32";
  if (!model || !rows || !clients || !rec || !workspace)
    return cw_error(FEDAVG_EINVAL, "%s: null model, rows, clients, rec or workspace", what);
  if (K < 1 || K > kCwMaxK) return cw_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kCwMaxK);
  if (D < 1 || D > kCwMaxD) return cw_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kCwMaxD);
  if (C < 2 || C > kCwMaxC) return cw_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kCwMaxC);
  const int64_t P = C * D + C;
  if (P > kCwMaxP)
    return cw_error(FEDAVG_EINVAL, "%s: P = %lld outside [1, %lld]", what, (long long)P, (long long)kCwMaxP);
  if (ld < P) return cw_error(FEDAVG_EINVAL, "%s: ld = %lld below P = %lld", what, (long long)ld, (long long)P);
  if (iters < 0 || iters > INT32_MAX) return cw_error(FEDAVG_EINVAL, "%s: negative iteration count", what);
  if (activation != 0 && activation != 1)
    return cw_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return cw_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return cw_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && iters > 0 && !coef) return cw_error(FEDAVG_EINVAL, "%s: null coef", what);
  const int64_t q = slices_per_group;
  if (q < 1 || q > cw_max_slices(C))
    return cw_error(FEDAVG_EINVAL, "%s: slices_per_group = %lld outside [1, %lld] at C = %lld", what, (long long)q,
                    (long long)cw_max_slices(C), (long long)C);
  if (misaligned(model, 4) || misaligned(rows, 4) || misaligned(clients, 8) || misaligned(rec, 8) ||
      (adam && misaligned(coef, 8)) || misaligned(workspace, 8))
    return cw_error(FEDAVG_EALIGN, "%s: model, rows must be 4-B, clients, rec, coef and workspace 8-B aligned", what);

  // ---- the table, read on the host where it lies
  const CwEntry* tab = static_cast<const CwEntry*>(clients);
  std::bitset<kCwMaxK> seen;
  bool dma = D % 4 == 0;
  int64_t N = 0;
  for (int64_t g = 0; g < K; ++g) {
    const CwEntry& e = tab[g];
    if (!e.x || !e.y) return cw_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kCwMaxB)
      return cw_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kCwMaxB);
    if (e.row < 0 || e.row >= K)
      return cw_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld outside [0, %lld)", what, (long long)g, (long long)e.row,
                      (long long)K);
    if (seen[e.row]) return cw_error(FEDAVG_EINVAL, "%s: entry %lld: row %lld used twice", what, (long long)g, (long long)e.row);
    seen[e.row] = true;
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return cw_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    dma = dma && !misaligned(e.x, 16);
    N += cw_groups(e.B, q);
  }
  if (workspace_bytes < cw_workspace(K, N, P, adam))
    return cw_error(FEDAVG_EINVAL, "%s: workspace of %lld bytes below the %lld of fedavg_client_wide_workspace_bytes",
                    what, (long long)workspace_bytes, (long long)cw_workspace(K, N, P, adam));

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return cw_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || !is_device_memory(rows) || !is_device_memory(workspace))
    return cw_error(FEDAVG_EINVAL, "%s: model, rows and workspace must be device memory", what);
  if (!is_device_memory(rec) && !is_pinned_host_memory(rec))
    return cw_error(FEDAVG_EINVAL, "%s: rec must be device or pinned host memory", what);
  if (adam && iters > 0) {
    if (!is_pinned_host_memory(coef)) return cw_error(FEDAVG_EINVAL, "%s: coef is not pinned host memory", what);
    for (int64_t t = 0; t < iters; ++t)
      if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
        return cw_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                        coef[kAdamCoefs * t + 1]);
  }
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return cw_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  const int64_t lds = 2 * kCwUnit * 4 + q * cw_dz_bytes(C);
  const auto grad = dma ? client_wide_grad_kernel<true> : client_wide_grad_kernel<false>;
  const auto step = adam ? client_wide_step_kernel<true> : client_wide_step_kernel<false>;
  {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(grad),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return cw_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }

  // ---- 1 + 4 * iters launches, nothing between them but the stream's order
  hipStream_t s = static_cast<hipStream_t>(stream);
  const CwLayout w = cw_layout(workspace, K, N, P, adam);
  const int NC = static_cast<int>(cw_chunks(P));
  const CwSetup su = {model, rows, tab, rec, w, ld, static_cast<int>(K), static_cast<int>(P), static_cast<int>(C),
                      static_cast<int>(q)};
  hipLaunchKernelGGL(client_wide_setup_kernel, dim3(static_cast<unsigned>(K + 1)), dim3(kLinThreads), 0, s, su);
  int rc = launch_status(g_cw_err, what);
  const CwGrad ga = {rows, w, ld, static_cast<int>(D), static_cast<int>(C), static_cast<int>(q), activation};
  CwSum sm = {rows, w, ld, static_cast<int>(K), static_cast<int>(P), NC, 0};
  CwStep sa = {rows, rec, w, {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, lr_ratio, ld,
               static_cast<float>(-lr),  // ATen: rounded once to opmath
               static_cast<int>(K), static_cast<int>(P), NC, form, 0, 0};
  const dim3 chunks(static_cast<unsigned>(NC), static_cast<unsigned>(K));
  for (int64_t ep = 0; ep < iters && rc == FEDAVG_OK; ++ep) {  // a refused launch is not followed by more of them
    hipLaunchKernelGGL(grad, dim3(static_cast<unsigned>(N)), dim3(kLinThreads), static_cast<size_t>(lds), s, ga);
    sm.ep = static_cast<int>(ep);
    hipLaunchKernelGGL(client_wide_sum_kernel, chunks, dim3(kLinThreads), 0, s, sm);
    if (adam)
      for (int j = 0; j < kAdamCoefs; ++j) sa.coef[j] = coef[kAdamCoefs * ep + j];
    sa.ep = static_cast<int>(ep);
    sa.last = ep + 1 == iters ? 1 : 0;
    hipLaunchKernelGGL(step, chunks, dim3(kLinThreads), 0, s, sa);
    hipLaunchKernelGGL(client_wide_track_kernel, dim3(static_cast<unsigned>(K)), dim3(64), 0, s, sa);
    rc = launch_status(g_cw_err, what);
  }
  return rc;
}

}  // extern "C"
