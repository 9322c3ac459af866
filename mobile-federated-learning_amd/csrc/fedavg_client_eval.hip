// fedavg_client_eval.hip -- libfedavg_amd_clienteval.so (include/
// fedavg_amd_clienteval.h): the evaluation of one linear softmax model on the
// whole dataset of every client (fedavg_trainer.py:461-529: a Client.local_test
// per client and set) in one call.
//
// Forward only, and not the training loop with the step removed.  There W
// changes every epoch, lives in registers split over D across eight waves, and
// the waves meet in LDS for the logits.  Here W is constant and x is read
// exactly once, so the split is over ROWS:
//
//   Work unit.  A chunk is a run of at most 256 rows of one client: 4 waves x 4
//   row tiles x 16 rows.  client_eval_setup_kernel turns the table's B into a
//   prefix table of chunk counts (and copies the table to device memory); the
//   persistent grid of client_eval_f32_kernel takes chunks blockIdx.x,
//   blockIdx.x + gridDim.x, ... and finds a chunk's client in that table.
//
//   W in LDS, once per workgroup: 16 classes x S floats, S = 16 ceil(D / 16) + 4,
//   classes from C on and columns from D on zero.  S / 4 is odd, so the 16
//   lanes of a 16-lane row, which read W[n][16 s + 4 q ..+3] for n = 0 .. 15,
//   touch 16 different 16-B bank groups: the B operand's one ds_read_b128 per
//   k-step has no bank conflict.
//
//   x from global memory straight into registers in the A-operand layout: lane
//   (i, q) loads x[row0 + i][16 s + 4 q ..+3], 16 B, nontemporal, and feeds the
//   four matrix instructions of k-step s (instruction j contracts columns
//   16 s + 4 q' + j, the permutation of client_stream_core.hpp).  No LDS copy and
//   no barrier in the k loop.  A wave carries 4 row tiles, so one LDS read of W
//   serves 16 matrix instructions, and two groups of kEvAhead k-steps of loads
//   are in flight.
//
//   Epilogue in registers: lane (n, q) holds z[4 q + r][n] of a tile; bias,
//   activation, classes >= C to -inf, then max-with-index and sum-of-exp over
//   the 16 lanes of a row by DPP butterflies.  Loss in fp64 and counts in
//   integers: a lane's rows in order, the wave's lanes by DPP, the waves in
//   order through LDS, into the CHUNK's partial; client_eval_finish_kernel adds
//   a client's chunks in order.  No atomics, no counters: the result depends
//   neither on the grid nor on the order of the table.
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include <bitset>

#include "client_linear_core.hpp"
#include "fedavg_amd_clienteval.h"

namespace {

thread_local ErrorState g_ev_err;

int ev_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_ev_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

constexpr int kEvMaxK = 4096, kEvMaxB = 16384;  // fedavg_client_cohort_limits'
static_assert(static_cast<int64_t>(kEvMaxB) * kLinMaxD <= (int64_t{1} << 24), "32-bit indexing");
constexpr int kEvThreads = 256, kEvWaves = kEvThreads / 64;
constexpr int kEvTiles = 4;                           // row tiles a wave carries (M)
constexpr int kEvChunk = 16 * kEvTiles * kEvWaves;    // rows of a chunk
constexpr int kEvAhead = 2;                           // k-steps per group of loads; two groups are in flight
constexpr int kEvPad = 4;                             // floats after the 16 ceil(D / 16) of an LDS row: S / 4 odd
static_assert(kEvChunk == 256, "the header's chunk");

// an entry of the client table, as the header lays it out
struct EvEntry {
  const float* x;
  const int64_t* y;
  int64_t B;
  int64_t slot;
};
static_assert(sizeof(EvEntry) == 32, "the header's 32-B entry");

// what a chunk leaves
struct EvPartial {
  double loss;
  int64_t correct, flag, unused;
};
static_assert(sizeof(EvPartial) == 32, "the header's 32-B partial");

__host__ __device__ inline int64_t ev_chunks(int64_t B) { return (B + kEvChunk - 1) / kEvChunk; }
inline int64_t ev_start_bytes(int64_t K) { return (4 * (K + 1) + 31) / 32 * 32; }

struct EvArgs {
  const float* model;
  const int* start;        // [K + 1]: entry g's chunks are start[g] .. start[g + 1] - 1
  const EvEntry* entries;  // the device copy of the table
  EvPartial* part;
  int K, D, C, act, nchunks, S, KS;
};

// ---------------------------------------------------------------- setup: the prefix table and the table's copy
__global__ __launch_bounds__(kEvThreads) void client_eval_setup_kernel(const EvEntry* tab, int K, int* start,
                                                                       EvEntry* copy) {
  __shared__ int sums[kEvThreads];
  const int t = threadIdx.x, per = (K + kEvThreads - 1) / kEvThreads;
  const int g0 = t * per < K ? t * per : K, g1 = g0 + per < K ? g0 + per : K;
  int s = 0;
  for (int g = g0; g < g1; ++g) s += static_cast<int>(ev_chunks(tab[g].B));
  sums[t] = s;
  __syncthreads();
  int pre = 0;
  for (int u = 0; u < t; ++u) pre += sums[u];
  for (int g = g0; g < g1; ++g) {
    const EvEntry e = tab[g];
    copy[g] = e;
    start[g] = pre;
    pre += static_cast<int>(ev_chunks(e.B));
  }
  if (g0 < K && g1 == K) start[K] = pre;  // the one thread whose run ends the table
}

// ---------------------------------------------------------------- DPP moves inside a 16-lane row
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ int ev_dpp(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ float ev_dpp(float v) {
  return __int_as_float(ev_dpp<CTRL>(__float_as_int(v)));
}

// torch.max's order: does (av, ai) come before (bv, bi)?  A NaN beats every number, the lower index wins a tie.
__device__ __forceinline__ bool ev_beats(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return an && (!bn || ai < bi);
  return av > bv || (av == bv && ai < bi);
}

template <int CTRL>
__device__ __forceinline__ void ev_max_step(float& mx, int& arg) {
  const float om = ev_dpp<CTRL>(mx);
  const int oa = ev_dpp<CTRL>(arg);
  const bool take = ev_beats(om, oa, mx, arg);
  mx = take ? om : mx;
  arg = take ? oa : arg;
}

// the sum of the 64 lanes' v, the same in every lane (wave_sum_dpp's moves)
__device__ __forceinline__ int ev_wave_sum(int v) {
  v += ev_dpp<0xB1>(v);        // quad_perm [1,0,3,2]
  v += ev_dpp<0x4E>(v);        // quad_perm [2,3,0,1]
  v += ev_dpp<0x141>(v);       // row_half_mirror
  v += ev_dpp<0x140>(v);       // row_mirror
  v += ev_dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1 and 3
  v += ev_dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

// ---------------------------------------------------------------- the forward kernel
// One group of kEvAhead k-steps of a wave's kEvTiles row tiles, as loaded
struct EvGroup {
  f32x4 v[kEvAhead][kEvTiles];
};

// x[.][col .. col + 3] of the lane's row of each tile.  Every load is issued, with no branch around it, so that
// nothing makes the compiler wait for the loads in flight: what lies past D or past the last k-step is read from
// `safe` (16 B of the workspace, always cached) and dropped by ev_mul.
template <bool VEC>
__device__ __forceinline__ void ev_load(EvGroup& g, const float* x, const float* safe, const int (&off)[kEvTiles],
                                        int s0, int KS, int q, int D) {
#pragma unroll
  for (int u = 0; u < kEvAhead; ++u) {
    const int s = s0 + u, col = 16 * s + 4 * q;
#pragma unroll
    for (int m = 0; m < kEvTiles; ++m) {
      if constexpr (VEC) {
        const float* p = s < KS && col < D ? x + off[m] + col : safe;
        g.v[u][m] = __builtin_nontemporal_load(to_global(reinterpret_cast<const f32x4*>(p)));
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* p = s < KS && col + j < D ? x + off[m] + col + j : safe;
          g.v[u][m][j] = __builtin_nontemporal_load(to_global(p));
        }
      }
    }
  }
}

__device__ __forceinline__ void ev_mul(f32x4 (&z)[kEvTiles], const EvGroup& g, const float* wl, int s0, int KS, int q,
                                       int D) {
#pragma unroll
  for (int u = 0; u < kEvAhead; ++u) {
    const int s = s0 + u, col = 16 * s + 4 * q;
    if (s < KS) {  // uniform, and around no load
      const f32x4 wv = *reinterpret_cast<const f32x4*>(wl + 16 * s);
#pragma unroll
      for (int m = 0; m < kEvTiles; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) z[m] = mfma4(col + j < D ? g.v[u][m][j] : 0.f, wv[j], z[m]);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kEvThreads) void client_eval_f32_kernel(const EvArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ws[];  // W: 16 classes of S floats
  __shared__ double red_loss[kEvWaves];
  __shared__ int red_cnt[kEvWaves], red_flag[kEvWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = lane & 15, q = lane >> 4;
  const int D = a.D, C = a.C, S = a.S, KS = a.KS;

  for (int idx = tid; idx < 16 * S; idx += kEvThreads) {
    const int c = idx / S, d = idx - c * S;
    ws[idx] = c < C && d < D ? a.model[c * D + d] : 0.f;
  }
  const float bias = n < C ? a.model[C * D + n] : 0.f;
  __syncthreads();
  const float* wl = ws + n * S + 4 * q;

  for (int c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    int lo = 0, hi = a.K;  // the chunk's entry: the last g with start[g] <= c
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.start[mid] <= c) lo = mid; else hi = mid;
    }
    const EvEntry e = a.entries[lo];
    const int B = static_cast<int>(e.B), row0 = (c - a.start[lo]) * kEvChunk + wave * (16 * kEvTiles);
    double loss = 0.0;
    int cnt = 0, flag = 0;

    if (row0 < B) {  // uniform in the wave: all 64 lanes run the DPP moves below
      int off[kEvTiles];
#pragma unroll
      for (int m = 0; m < kEvTiles; ++m) {
        const int r = row0 + 16 * m + n;
        off[m] = (r < B ? r : B - 1) * D;  // a row past the batch reads the last row; its logits are dropped
      }
      f32x4 z[kEvTiles];
#pragma unroll
      for (int m = 0; m < kEvTiles; ++m) z[m] = f32x4{0.f, 0.f, 0.f, 0.f};
      EvGroup ga, gb;
      const float* safe = reinterpret_cast<const float*>(a.start);
      ev_load<VEC>(ga, e.x, safe, off, 0, KS, q, D);
      for (int s0 = 0; s0 < KS; s0 += 2 * kEvAhead) {
        ev_load<VEC>(gb, e.x, safe, off, s0 + kEvAhead, KS, q, D);
        ev_mul(z, ga, wl, s0, KS, q, D);
        ev_load<VEC>(ga, e.x, safe, off, s0 + 2 * kEvAhead, KS, q, D);
        ev_mul(z, gb, wl, s0 + kEvAhead, KS, q, D);
      }

      const auto* yg = to_global(e.y);
#pragma unroll
      for (int m = 0; m < kEvTiles; ++m) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = row0 + 16 * m + 4 * q + r;
          const bool live = row < B;
          const int64_t y = yg[live ? row : B - 1];  // past the batch: the last label, read and dropped
          const bool ok = y >= 0 && y < C;
          const float zc = z[m][r] + bias;
          float act = a.act ? 1.0f / (1.0f + __builtin_expf(-zc)) : zc;
          act = n < C ? act : -INFINITY;
          float mx = act;
          int arg = n;
          ev_max_step<0xB1>(mx, arg);
          ev_max_step<0x4E>(mx, arg);
          ev_max_step<0x141>(mx, arg);
          ev_max_step<0x140>(mx, arg);
          float se = n < C ? __builtin_expf(act - mx) : 0.f;
          se += ev_dpp<0xB1>(se);
          se += ev_dpp<0x4E>(se);
          se += ev_dpp<0x141>(se);
          se += ev_dpp<0x140>(se);
          const float ls = (act - mx) - __builtin_logf(se);  // log_softmax of class n
          const int yi = static_cast<int>(y);
          loss += live && ok && n == yi ? static_cast<double>(-ls) : 0.0;
          cnt += live && ok && n == 0 && arg == yi ? 1 : 0;
          flag |= live && !ok ? 1 : 0;
        }
      }
      loss = wave_sum_dpp(loss);
      cnt = ev_wave_sum(cnt);
      flag = ev_wave_sum(flag);
    }
    if (lane == 0) {
      red_loss[wave] = loss;
      red_cnt[wave] = cnt;
      red_flag[wave] = flag;
    }
    __syncthreads();
    if (tid == 0) {
      double l = red_loss[0];
      int k = red_cnt[0], f = red_flag[0];
#pragma unroll
      for (int w = 1; w < kEvWaves; ++w) {
        l += red_loss[w];
        k += red_cnt[w];
        f += red_flag[w];
      }
      a.part[c] = EvPartial{l, k, f ? 1 : 0, 0};
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------- finish: a client's chunks in order, one thread each
__global__ __launch_bounds__(kEvThreads) void client_eval_finish_kernel(const int* start, const EvEntry* entries,
                                                                        const EvPartial* part, int K, double* rec) {
  const int g = blockIdx.x * kEvThreads + threadIdx.x;
  if (g >= K) return;
  const EvEntry e = entries[g];
  double loss = 0.0;
  int64_t cnt = 0, flag = 0;
  for (int c = start[g]; c < start[g + 1]; ++c) {
    loss += part[c].loss;
    cnt += part[c].correct;
    flag |= part[c].flag;
  }
  double* r = rec + 4 * e.slot;
  r[0] = loss;
  r[1] = static_cast<double>(cnt);
  r[2] = static_cast<double>(flag);
  r[3] = static_cast<double>(e.B);
}

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// workgroups the chip keeps resident with `lds` bytes each, 0 = not granted
template <bool VEC>
int64_t ev_resident(int64_t lds) {
  return static_cast<int64_t>(lds_blocks_per_cu(client_eval_f32_kernel<VEC>, kEvThreads, lds)) * cu_count();
}

// the table's checks that need no HIP call; *chunks and *vec as found
int ev_check_table(const char* what, const EvEntry* tab, int64_t K, int64_t* chunks, bool* vec) {
  std::bitset<kEvMaxK> seen;
  *chunks = 0;
  for (int64_t g = 0; g < K; ++g) {
    const EvEntry& e = tab[g];
    if (!e.x || !e.y) return ev_error(FEDAVG_EINVAL, "%s: entry %lld: null x or y", what, (long long)g);
    if (e.B < 1 || e.B > kEvMaxB)
      return ev_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g, (long long)e.B,
                      kEvMaxB);
    if (e.slot < 0 || e.slot >= K)
      return ev_error(FEDAVG_EINVAL, "%s: entry %lld: slot %lld outside [0, %lld)", what, (long long)g,
                      (long long)e.slot, (long long)K);
    if (seen[e.slot])
      return ev_error(FEDAVG_EINVAL, "%s: entry %lld: slot %lld used twice", what, (long long)g, (long long)e.slot);
    seen[e.slot] = true;
    if (misaligned(e.x, 4) || misaligned(e.y, 8))
      return ev_error(FEDAVG_EALIGN, "%s: entry %lld: x must be 4-B, y 8-B aligned", what, (long long)g);
    *chunks += ev_chunks(e.B);
    *vec = *vec && !misaligned(e.x, 16);
  }
  return 0;
}

}  // namespace

extern "C" {

int fedavg_clienteval_abi_version(void) { return 1; }

const char* fedavg_clienteval_last_error(void) { return g_ev_err.c_str(); }

void fedavg_client_eval_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c) {
  if (max_k) *max_k = kEvMaxK;
  if (max_b) *max_b = kEvMaxB;
  if (max_d) *max_d = kLinMaxD;
  if (max_c) *max_c = kLinMaxC;
}

int64_t fedavg_client_eval_workspace_bytes(const void* clients, int64_t K, int64_t D) {
  const char* what = "fedavg_client_eval_workspace_bytes";
  if (!clients) return ev_error(FEDAVG_EINVAL, "%s: null clients", what);
  if (K < 1 || K > kEvMaxK) return ev_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kEvMaxK);
  if (D < 1 || D > kLinMaxD) return ev_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  const EvEntry* tab = static_cast<const EvEntry*>(clients);
  int64_t chunks = 0;
  for (int64_t g = 0; g < K; ++g) {
    if (tab[g].B < 1 || tab[g].B > kEvMaxB)
      return ev_error(FEDAVG_EINVAL, "%s: entry %lld: B = %lld outside [1, %d]", what, (long long)g,
                      (long long)tab[g].B, kEvMaxB);
    chunks += ev_chunks(tab[g].B);
  }
  return ev_start_bytes(K) + 32 * K + 32 * chunks;
}

int fedavg_client_eval_f32(const float* model, const void* clients, int64_t K, int64_t D, int64_t C, int activation,
                           double* rec, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* what = "fedavg_client_eval_f32";
  if (!model || !clients || !rec || !workspace)
    return ev_error(FEDAVG_EINVAL, "%s: null model, clients, rec or workspace", what);
  if (K < 1 || K > kEvMaxK) return ev_error(FEDAVG_EINVAL, "%s: K = %lld outside [1, %d]", what, (long long)K, kEvMaxK);
  if (D < 1 || D > kLinMaxD) return ev_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return ev_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  if (activation != 0 && activation != 1)
    return ev_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (misaligned(model, 4) || misaligned(clients, 8) || misaligned(rec, 8) || misaligned(workspace, 16))
    return ev_error(FEDAVG_EALIGN, "%s: model must be 4-B, clients and rec 8-B, workspace 16-B aligned", what);

  // ---- the table, read on the host where it lies
  const EvEntry* tab = static_cast<const EvEntry*>(clients);
  int64_t chunks = 0;
  bool vec = D % 4 == 0;
  if (const int rc = ev_check_table(what, tab, K, &chunks, &vec)) return rc;
  const int64_t off_entries = ev_start_bytes(K), off_part = off_entries + 32 * K, need = off_part + 32 * chunks;
  if (workspace_bytes < need)
    return ev_error(FEDAVG_EINVAL, "%s: workspace of %lld bytes below the %lld needed", what, (long long)workspace_bytes,
                    (long long)need);

  // ---- the kinds of memory
  if (!is_pinned_host_memory(clients)) return ev_error(FEDAVG_EINVAL, "%s: clients is not pinned host memory", what);
  if (!is_device_memory(model) || !is_device_memory(workspace))
    return ev_error(FEDAVG_EINVAL, "%s: model and workspace must be device memory", what);
  if (!is_device_memory(rec) && !is_pinned_host_memory(rec))
    return ev_error(FEDAVG_EINVAL, "%s: rec must be device or pinned host memory", what);
  for (int64_t g = 0; g < K; ++g)
    if (!is_device_memory(tab[g].x) || !is_device_memory(tab[g].y))
      return ev_error(FEDAVG_EINVAL, "%s: entry %lld: x and y must be device memory", what, (long long)g);

  char* base = static_cast<char*>(workspace);
  int* start = reinterpret_cast<int*>(base);
  EvEntry* entries = reinterpret_cast<EvEntry*>(base + off_entries);
  EvPartial* part = reinterpret_cast<EvPartial*>(base + off_part);
  const int64_t KS = (D + 15) / 16, S = 16 * KS + kEvPad;
  const EvArgs a = {model, start, entries, part, static_cast<int>(K), static_cast<int>(D), static_cast<int>(C),
                    activation, static_cast<int>(chunks), static_cast<int>(S), static_cast<int>(KS)};
  const int64_t lds = 16 * S * 4, resident = vec ? ev_resident<true>(lds) : ev_resident<false>(lds);
  if (resident <= 0) return ev_error(FEDAVG_EINVAL, "%s: %lld bytes of LDS are not granted", what, (long long)lds);
  const dim3 grid(static_cast<unsigned>(chunks < resident ? chunks : resident));  // persistent
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(client_eval_setup_kernel, dim3(1), dim3(kEvThreads), 0, s, tab, static_cast<int>(K), start, entries);
  if (const int rc = launch_status(g_ev_err, what)) return rc;
  if (vec)
    hipLaunchKernelGGL(client_eval_f32_kernel<true>, grid, dim3(kEvThreads), static_cast<size_t>(lds), s, a);
  else
    hipLaunchKernelGGL(client_eval_f32_kernel<false>, grid, dim3(kEvThreads), static_cast<size_t>(lds), s, a);
  if (const int rc = launch_status(g_ev_err, what)) return rc;
  hipLaunchKernelGGL(client_eval_finish_kernel, dim3(grid_for(K, kEvThreads)), dim3(kEvThreads), 0, s, start, entries,
                     part, static_cast<int>(K), rec);
  return launch_status(g_ev_err, what);
}

}  // extern "C"
