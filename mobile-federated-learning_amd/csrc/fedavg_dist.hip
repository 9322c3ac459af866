// fedavg_dist.hip -- the post-aggregate client distance pass
// (fedavg_trainer.py:291) of libfedavg_amd.so.
#include "common.hpp"
#include "dist_plan.hpp"
#include "window.hpp"

namespace {
using namespace fedavg_impl;

// ---------------------------------------------------------------------------
// Post-aggregate client distances (fedavg_trainer.py:291): for every client i
//   sumsq[i] = sum_p fl32(x_i[p] - g[p])^2
// with the difference formed in fp32 exactly as the reference's
// `w[para] - w_glob[para]` forms it, each square exact in fp64 and the sum in
// fp64 (deterministic order: per-wave partials, then a fixed-order finalize).
// The reference's ATen fp32 norm accumulates in fp32 SIMD lanes; this is the
// accurate value it approximates.  HBM-read bound like the reduce: 4K+4 B per
// element.  Thread = C 16-B column slices (slice j at base + tid + 256j).
// ---------------------------------------------------------------------------
// acc + the exact squares of d's four lanes, in fp64 with fused multiply-adds
// (this pass is tolerance-pinned, not bit-pinned: a fused square-add rounds
// once, so it is closer to the exact sum, and it halves the fp64 work)
__device__ __forceinline__ double sq4_add(double acc, f32x4 d) {
  const double x = d.x, y = d.y, z = d.z, w = d.w;
  acc = __builtin_fma(x, x, acc);
  acc = __builtin_fma(y, y, acc);
  acc = __builtin_fma(z, z, acc);
  return __builtin_fma(w, w, acc);
}

__device__ __forceinline__ double wave_sum(double v) { return wave_sum_dpp(v); }

// Block b of a launch covers C*256 column slices starting at slice
// b*C*256 of that launch's window; its waves write partials at global wave
// index wave_base + b*4 + wave.  U client rows are loaded per batch.
template <int U, int C>
__global__ __launch_bounds__(kBlock) void client_sqdist_f32x4_kernel(
    const f32x4* __restrict__ X, int K, int64_t ld4, int64_t nvec, int tail, const f32x4* __restrict__ G,
    double* __restrict__ partials, int64_t nwaves, int64_t wave_base) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_id = wave_base + static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock * C + threadIdx.x;
  f32x4 g[C];
  int nv[C];  // valid elements of slice j (0..4): padding lanes never contribute
  bool valid[C];
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int64_t v = base + static_cast<int64_t>(j) * kBlock;
    valid[j] = v < nvec;
    g[j] = valid[j] ? G[v] : f32x4{0.f, 0.f, 0.f, 0.f};
    nv[j] = !valid[j] ? 0 : (tail != 0 && v == nvec - 1 ? tail : 4);
  }
  const f32x4* col = X + base;
  for (int k = 0; k < K; k += U) {
    const int rows = (K - k) < U ? (K - k) : U;
    f32x4 xs[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < C; ++j)
        xs[u][j] = (u < rows && valid[j]) ? ld<true>(col + static_cast<int64_t>(k + u) * ld4 + j * kBlock) : g[j];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u >= rows) break;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < C; ++j) {
        f32x4 d = xs[u][j] - g[j];  // fp32 difference, as the reference forms it
        if (nv[j] < 4) {            // select (not multiply): padding may hold NaN/inf
          d.x = nv[j] > 0 ? d.x : 0.f;
          d.y = nv[j] > 1 ? d.y : 0.f;
          d.z = nv[j] > 2 ? d.z : 0.f;
          d.w = 0.f;
        }
        acc = sq4_add(acc, d);
      }
      acc = wave_sum(acc);
      if (lane == 0) partials[static_cast<int64_t>(k + u) * nwaves + wave_id] = acc;
    }
  }
}

// The same pass through buffer descriptors, split by column group.  A FULL
// group (every slice valid, no P % 4 tail) reads client row k through one
// descriptor whose base sits in SGPRs, with each lane's slice as a 32-bit
// offset shared by every row, and forms d = x - g with no masking at all --
// the reduce's register budget (reduce_f32x4_buf_kernel) plus the group's
// model slice g.  The ragged last group keeps per-slice masks and a record
// count that ends at the window's last float4 (lanes past it read 0).  Same
// per-wave partial layout as client_sqdist_f32x4_kernel<U, C>.
template <int U, int C>
__device__ __forceinline__ void sqdist_rows_store(double acc, double* partials, int64_t row, int64_t nwaves,
                                                  int64_t wave_id) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) partials[row * nwaves + wave_id] = acc;
}

// sum over a row's C slices of fl32(x - g)^2 in fp64, in ACC interleaved
// chains (slice j feeds chain j % ACC, the chains add pairwise at the end):
// ACC = 1 is one dependent chain of 4C fused square-adds per row
template <int C, int ACC>
__device__ __forceinline__ double sq_row(const f32x4 (&x)[C], const f32x4 (&g)[C]) {
  double a[ACC];
#pragma unroll
  for (int i = 0; i < ACC; ++i) a[i] = 0.0;
#pragma unroll
  for (int j = 0; j < C; ++j) a[j % ACC] = sq4_add(a[j % ACC], x[j] - g[j]);  // fp32 difference, as the reference
#pragma unroll
  for (int w = 1; w < ACC; w *= 2) {
#pragma unroll
    for (int i = 0; i + w < ACC; i += 2 * w) a[i] += a[i + w];
  }
  return a[0];
}

// STYLE L > 0 (probe): each batch's U x C loads and squares interleaved in
// (row, slice) order with at most L loads of the wave in flight, as the
// zero-copy reduce's unit loop (fedavg_segments.hip, STYLE 2)
template <int U, int C, int MINW = 1, int ACC = 1, int STYLE = 0>
__global__ __launch_bounds__(kBlock, MINW) void client_sqdist_buf_kernel(
    const f32x4* __restrict__ X, int K, int64_t ld4, int64_t nvec, int tail, const f32x4* __restrict__ G,
    double* __restrict__ partials, int64_t nwaves, int64_t wave_base) {
  const int64_t wave_id = wave_base + static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  constexpr int64_t span = static_cast<int64_t>(kBlock) * C;
  const int64_t blk0 = static_cast<int64_t>(blockIdx.x) * span;
  uint32_t off[C];
#pragma unroll
  for (int j = 0; j < C; ++j) off[j] = 16u * (threadIdx.x + j * kBlock);
  if (blk0 + span < nvec || (blk0 + span == nvec && tail == 0)) {
    constexpr int bytes = static_cast<int>(span * 16);
    f32x4 g[C];
    {
      const __amdgpu_buffer_rsrc_t rg = uniform_rsrc(G + blk0, bytes);
#pragma unroll
      for (int j = 0; j < C; ++j) g[j] = ld_rsrc_nt(rg, off[j]);
    }
    if constexpr (U == 0) {  // one row in flight while the previous one is summed
      const auto load_row = [&](f32x4 (&x)[C], int row) {
        const __amdgpu_buffer_rsrc_t r = uniform_rsrc(X + static_cast<int64_t>(row) * ld4 + blk0, bytes);
#pragma unroll
        for (int j = 0; j < C; ++j) x[j] = ld_rsrc_nt(r, off[j]);
      };
      f32x4 a[C], b[C];
      load_row(a, 0);
      int k = 0;
      for (; k + 2 <= K; k += 2) {
        load_row(b, k + 1);
        sqdist_rows_store<1, C>(sq_row<C, ACC>(a, g), partials, k, nwaves, wave_id);
        if (k + 2 < K) load_row(a, k + 2);
        sqdist_rows_store<1, C>(sq_row<C, ACC>(b, g), partials, k + 1, nwaves, wave_id);
      }
      if (k < K) sqdist_rows_store<1, C>(sq_row<C, ACC>(a, g), partials, k, nwaves, wave_id);
      return;
    }
    constexpr int UU = U > 0 ? U : 1;
    int k = 0;
    if constexpr (STYLE > 0) {
      constexpr int L = STYLE, N = UU * C;
      for (; k + UU <= K; k += UU) {
        __amdgpu_buffer_rsrc_t rr[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) rr[u] = uniform_rsrc(X + static_cast<int64_t>(k + u) * ld4 + blk0, bytes);
        double a[UU][ACC];
#pragma unroll
        for (int u = 0; u < UU; ++u)
#pragma unroll
          for (int c = 0; c < ACC; ++c) a[u][c] = 0.0;
        f32x4 x[N];
#pragma unroll
        for (int i = 0; i < N + L; ++i) {
          if (i < N) x[i] = ld_rsrc_nt(rr[i / C], off[i % C]);
          if (i >= L) {
            const int j = i - L;
            a[j / C][(j % C) % ACC] = sq4_add(a[j / C][(j % C) % ACC], x[j] - g[j % C]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
#pragma unroll
          for (int w = 1; w < ACC; w *= 2) {
#pragma unroll
            for (int c = 0; c + w < ACC; c += 2 * w) a[u][c] += a[u][c + w];
          }
          sqdist_rows_store<U, C>(a[u][0], partials, k + u, nwaves, wave_id);
        }
      }
    }
    for (; k + UU <= K; k += UU) {
      f32x4 xs[UU][C];
#pragma unroll
      for (int u = 0; u < UU; ++u) {
        const __amdgpu_buffer_rsrc_t r = uniform_rsrc(X + static_cast<int64_t>(k + u) * ld4 + blk0, bytes);
#pragma unroll
        for (int j = 0; j < C; ++j) xs[u][j] = ld_rsrc_nt(r, off[j]);
      }
#pragma unroll
      for (int u = 0; u < UU; ++u) sqdist_rows_store<U, C>(sq_row<C, ACC>(xs[u], g), partials, k + u, nwaves, wave_id);
    }
    for (; k < K; ++k) {
      const __amdgpu_buffer_rsrc_t r = uniform_rsrc(X + static_cast<int64_t>(k) * ld4 + blk0, bytes);
      f32x4 x[C];
#pragma unroll
      for (int j = 0; j < C; ++j) x[j] = ld_rsrc_nt(r, off[j]);
      sqdist_rows_store<U, C>(sq_row<C, ACC>(x, g), partials, k, nwaves, wave_id);
    }
    return;
  }
  // ragged last group: masked slices, record count ends at the last float4
  const int64_t left = nvec - blk0;
  const int bytes = static_cast<int>((left < span ? left : span) * 16);
  int nv[C];  // valid elements of slice j (0..4): padding lanes never contribute
  f32x4 g[C];
  {
    const __amdgpu_buffer_rsrc_t rg = uniform_rsrc(G + blk0, bytes);
#pragma unroll
    for (int j = 0; j < C; ++j) {
      const int64_t v = blk0 + threadIdx.x + static_cast<int64_t>(j) * kBlock;
      nv[j] = v >= nvec ? 0 : (tail != 0 && v == nvec - 1 ? tail : 4);
      g[j] = ld_rsrc_nt(rg, off[j]);
    }
  }
  for (int k = 0; k < K; ++k) {
    const __amdgpu_buffer_rsrc_t r = uniform_rsrc(X + static_cast<int64_t>(k) * ld4 + blk0, bytes);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < C; ++j) {
      f32x4 d = ld_rsrc_nt(r, off[j]) - g[j];
      if (nv[j] < 4) {  // select (not multiply): padding may hold NaN/inf
        d.x = nv[j] > 0 ? d.x : 0.f;
        d.y = nv[j] > 1 ? d.y : 0.f;
        d.z = nv[j] > 2 ? d.z : 0.f;
        d.w = 0.f;
      }
      acc = sq4_add(acc, d);
    }
    sqdist_rows_store<U, C>(acc, partials, k, nwaves, wave_id);
  }
}

// ---------------------------------------------------------------------------
// :291 for fp64 / fp16 / bf16 keys.  `w[para] - w_glob[para]` forms the
// difference in the key's own dtype (ATen: fp64 math for fp64; fp32 opmath
// rounded to fp16/bf16 for the 16-bit types), torch.cat then widens it
// exactly to the promoted dtype, and the norm squares and sums.  Here: the
// difference with the reference's rounding, then exact-ish fp64 squares and
// sum (fused square-adds), same per-wave partial layout and fixed-order
// finalize as the fp32 pass.  16-B slices: 2 fp64 or 8 fp16/bf16 elements.
// ---------------------------------------------------------------------------
struct DistF64 {
  using vec = f64x2;
  static constexpr int kLanes = 2;
  __device__ static double sq_add(double acc, vec x, vec g, int nv) {
    const vec d = x - g;  // fp64 difference, as the reference forms it
    if (nv > 0) acc = __builtin_fma(d.x, d.x, acc);
    if (nv > 1) acc = __builtin_fma(d.y, d.y, acc);
    return acc;
  }
};

template <typename R>
struct DistHalf {
  using vec = u16x8;
  static constexpr int kLanes = 8;
  __device__ static double sq_add(double acc, vec x, vec g, int nv) {
    u32x4 xu, gu;
    __builtin_memcpy(&xu, &x, 16);
    __builtin_memcpy(&gu, &g, 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // fl16(fl32(x) - fl32(g)): ATen's opmath subtraction rounded to the
      // key's 16-bit type, then widened exactly
      const f32x2 d = R::unpack(R::pack(opaque2(R::unpack(xu[j]) - R::unpack(gu[j]))));
      const double a = d.x, b = d.y;
      if (2 * j < nv) acc = __builtin_fma(a, a, acc);
      if (2 * j + 1 < nv) acc = __builtin_fma(b, b, acc);
    }
    return acc;
  }
};

template <class D, int U, int C>
__global__ __launch_bounds__(kBlock) void client_sqdist_vec_kernel(
    const typename D::vec* __restrict__ X, int K, int64_t ldv, int64_t nvec, int tail,
    const typename D::vec* __restrict__ G, double* __restrict__ partials, int64_t nwaves) {
  using vec = typename D::vec;
  const int lane = threadIdx.x & 63;
  const int64_t wave_id = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kBlock * C + threadIdx.x;
  vec g[C];
  int nv[C];  // valid elements of slice j: padding lanes never contribute
#pragma unroll
  for (int j = 0; j < C; ++j) {
    const int64_t v = base + static_cast<int64_t>(j) * kBlock;
    nv[j] = v >= nvec ? 0 : (tail != 0 && v == nvec - 1 ? tail : D::kLanes);
    g[j] = nv[j] > 0 ? G[v] : vec{};
  }
  const vec* col = X + base;
  for (int k = 0; k < K; k += U) {
    const int rows = (K - k) < U ? (K - k) : U;
    vec xs[U][C];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < C; ++j)
        xs[u][j] = (u < rows && nv[j] > 0) ? ld<true>(col + static_cast<int64_t>(k + u) * ldv + j * kBlock) : g[j];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u >= rows) break;
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < C; ++j) acc = D::sq_add(acc, xs[u][j], g[j], nv[j]);
      acc = wave_sum(acc);
      if (lane == 0) partials[static_cast<int64_t>(k + u) * nwaves + wave_id] = acc;
    }
  }
}

// sumsq[k] = sum over waves of partials[k][*], fixed order (block per client).
__global__ __launch_bounds__(kBlock) void client_sqdist_finalize_kernel(const double* __restrict__ partials,
                                                                        int64_t nwaves, double* __restrict__ out) {
  __shared__ double red[kBlock];
  const int64_t k = blockIdx.x;
  double s = 0.0;
  for (int64_t w = threadIdx.x; w < nwaves; w += kBlock) s += partials[k * nwaves + w];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[k] = red[0];
}

// ---------------------------------------------------------------------------
// Aggregate (:450-457) and :291 in ONE pass over the client rows.  The
// reference reads every client's update twice per round: once to average it
// (:217) and once to measure ||w_i - w_glob|| (:291).  Both passes are
// HBM-read bound on the same K x P bytes, so fusing them halves the round's
// traffic -- if every column's K values are still on chip when that column's
// average is known.  A workgroup therefore owns tiles of S columns x all K
// rows staged in LDS (K x S x 4 bytes: 25.6 KB for K = 100, S = 64):
//   1. every row segment lands in LDS by LDS-DMA (global_load_lds_dwordx4,
//      1 KiB per wave instruction, no VGPR round trip).  The 16-B slots of
//      row r are XOR-swizzled by (r & 7): slot j holds the row's slice
//      j ^ (r & 7) (the swizzle is in the per-lane GLOBAL address; LDS stays
//      linear, as LDS-DMA requires), so threads reading one slice of 8
//      consecutive rows hit 8 different bank groups;
//   2. one thread per column runs the reference's sequential chain over the
//      K rows (fl32 products and sums in client order: the bits of
//      fedavg_reduce_f32) and stores the average to `out` and to LDS;
//   3. thread t owns row t % K and the slices t / K, t / K + q, ... (q =
//      256 / K threads per row), and adds fl32(x - g)^2 in fp64 to ONE
//      register accumulator that lives across all of the workgroup's tiles.
//      At the end the q accumulators of a row are added in a fixed order.
// A thread keeps one fp64 accumulator instead of one per row, so the kernel
// is LDS-bound, not register-bound: K = 100 x 64 columns runs 6 workgroups
// per CU.  Workgroups are persistent (grid = resident workgroups) and walk the
// tiles with a grid stride, so the running workgroups sweep one compact
// window of every row, as the round-split row reduce does.
// partials[k][workgroup], then the fixed-order finalize: deterministic.
// K <= 128 (q >= 2).
// ---------------------------------------------------------------------------

// rows -> LDS for the tile at column c0: slot i = row * V + j (LDS byte
// 16 i from `buf`) holds slice j ^ (row & 7) of the row segment
// Load slots per thread at the widest K each tile width serves (fused_cols):
// 128 x 64, 64 x 128, 32 x 256 columns
constexpr int kFusedSlots = 8;

// The byte offset (row * ld + slice) of each of this thread's load slots,
// the same for every tile: computed once per workgroup, so a tile's loads
// cost one 64-bit add each instead of the row / slice / swizzle arithmetic
template <int S>
struct FusedSlots {
  int64_t off[kFusedSlots];
};

template <int S>
__device__ __forceinline__ FusedSlots<S> fused_slots_of(int K, int64_t ld) {
  constexpr int V = S / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  FusedSlots<S> sl;
#pragma unroll
  for (int m = 0; m < kFusedSlots; ++m) {
    const int i = wave * 64 + m * kBlock + lane;
    const int row = i / V;
    const int c = (i % V) ^ (row & 7);
    sl.off[m] = (static_cast<int64_t>(row) * ld + 4 * c) * 4;
  }
  return sl;
}

// a full tile's loads through the precomputed slots (the ragged last tile
// takes fused_load_tile, which masks slices past the model's end)
template <int S>
__device__ __forceinline__ void fused_load_full(const float* __restrict__ X, int K, int64_t c0,
                                                const FusedSlots<S>& sl, float* buf) {
  constexpr int V = S / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nload = K * V;
  const char* base = reinterpret_cast<const char*>(X + c0);
#pragma unroll
  for (int m = 0; m < kFusedSlots; ++m) {
    const int i0 = wave * 64 + m * kBlock;
    if (i0 < nload && i0 + lane < nload)
      __builtin_amdgcn_global_load_lds((fused_gbl_t)(base + sl.off[m]), (fused_lds_t)(buf + 4 * i0), 16, 0, 2 /* nt */);
  }
}

template <int S>
__device__ __forceinline__ void fused_load_tile(const float* __restrict__ X, int K, int64_t ld, int64_t P, int64_t c0,
                                                float* buf) {
  constexpr int V = S / 4;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nload = K * V;
  const int ncols = P - c0 < S ? static_cast<int>(P - c0) : S;
  const int nv4 = (ncols + 3) >> 2;  // slices holding valid columns (the last may run into the row padding)
  for (int i0 = wave * 64; i0 < nload; i0 += kBlock) {
    const int i = i0 + lane;
    const int row = i / V;
    const int c = (i % V) ^ (row & 7);
    if (i < nload && c < nv4)
      __builtin_amdgcn_global_load_lds((fused_gbl_t)(X + static_cast<int64_t>(row) * ld + c0 + 4 * c),
                                       (fused_lds_t)(buf + 4 * i0), 16, 0, 2 /* nt */);
  }
}


// (the fourth template argument was the retired loads-only probe: always
// false, it stays because the pinned instance names carry it)
template <int S, bool DB, int RW = 0, bool = false, int RM = 1>
__global__ __launch_bounds__(kBlock) void reduce_sqdist_f32_kernel(const float* __restrict__ X, int K, int64_t ld,
                                                                   int64_t P, int64_t ntiles,
                                                                   const float* __restrict__ W,
                                                                   float* __restrict__ out,
                                                                   double* __restrict__ partials) {
  static_assert(S == 64 || S == 128 || S == 256, "tile widths: 64, 128 or 256 columns");
  // one tile buffer [K][S] (swizzled slots) -- two when DB -- then the tile's average [S]
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tile_floats = K * S;
  float* gs = lds + (DB ? 2 : 1) * tile_floats;
  double acc[RM][4];  // four chains per row this thread owns (one per lane of a 16-B slice)
#pragma unroll
  for (int m = 0; m < RM; ++m) acc[m][0] = acc[m][1] = acc[m][2] = acc[m][3] = 0.0;
  double acc_rows[RW > 0 ? RW : 1];      // RW > 0: one accumulator per row of this wave
#pragma unroll
  for (int r = 0; r < (RW > 0 ? RW : 1); ++r) acc_rows[r] = 0.0;
  const FusedSlots<S> slots = fused_slots_of<S>(K, ld);
  int cur = 0;
  if (DB && static_cast<int64_t>(blockIdx.x) < ntiles)
    fused_load_tile<S>(X, K, ld, P, static_cast<int64_t>(blockIdx.x) * S, lds);
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    float* tile = lds + cur * tile_floats;
    const int64_t c0 = t * S;
    const int ncols = P - c0 < S ? static_cast<int>(P - c0) : S;
    if constexpr (DB) {
      barrier_loads();  // this tile has landed; every wave is done with the other buffer
      // 1. the next tile's rows stream into the other buffer while this one is used
      if (t + gridDim.x < ntiles) fused_load_tile<S>(X, K, ld, P, (t + gridDim.x) * S, lds + (cur ^ 1) * tile_floats);
    } else {
      if (ncols == S && !RW && K * (S / 4) <= kFusedSlots * kBlock)  // 1. rows -> LDS
        fused_load_full<S>(X, K, c0, slots, tile);
      else
        fused_load_tile<S>(X, K, ld, P, c0, tile);
      barrier_loads();
    }
    fused_average<S>(tile, gs, K, W, ncols, out + c0);  // 2. the average of each column
    barrier_lds();
    if constexpr (RW > 0) {
      // 3'. rows wave + 4r (r < RW), S / 64 adjacent columns per lane, one
      //     register accumulator per row
      constexpr int PER = S / 64;
#pragma unroll
      for (int r = 0; r < RW; ++r) {
        const int row = (threadIdx.x >> 6) + 4 * r;
        if (row < K) {
          const int c = (threadIdx.x & 63) * PER;
          const float* x = tile + row * S + ((((c >> 2) ^ (row & 7))) << 2) + (c & 3);
#pragma unroll
          for (int j = 0; j < PER; ++j) {
            const float d = x[j] - gs[c + j];  // fp32 difference, as the reference forms it
            const double dd = c + j < ncols ? static_cast<double>(d) : 0.0;  // select: padding may hold NaN/inf
            acc_rows[r] = __builtin_fma(dd, dd, acc_rows[r]);
          }
        }
      }
    } else {
      fused_squares<S, RM>(tile, gs, K, ncols, acc);  // 3. :291 squares of this thread's rows over its slices
    }
    if constexpr (DB)
      cur ^= 1;
    else
      barrier_lds();  // the tile is read out before the next one lands
  }
  if constexpr (RW > 0) {
#pragma unroll
    for (int r = 0; r < RW; ++r) {
      const int row = (threadIdx.x >> 6) + 4 * r;
      if (row < K) {
        const double sr = wave_sum_dpp(acc_rows[r]);
        if ((threadIdx.x & 63) == 0) partials[static_cast<int64_t>(row) * gridDim.x + blockIdx.x] = sr;
      }
    }
    return;
  }
  fused_finish<RM>(lds, acc, K, partials);
}

// (The LDS-DMA kernel serves 17-128 rows in production, fused_plan in dist_plan.hpp.
// Round 2 ran it up to 300 clients with two rows per thread above 256:
// 200 x 10M 2.74 -> 1.84 ms, 300 x 5M 1.96 -> 1.58, but 500 x 11.2M 10.8 vs
// 7.26 ms for the two passes; profiles/r02/fused/fused_many_clients*_probe.jsonl.)

// One call of the fused pass as its launchers take it: the entry point's
// arguments (partials = the workspace)
struct FusedCall {
  const float* clients;
  int64_t K, P, ld;
  const float* weights;
  float* out;
  double* partials;
  int64_t partial_elems;
  double* sumsq;
  hipStream_t s;
  const char* what;
};

const LaunchCtx kRowsLaunch{set_error, launch_status, "%s: workspace needs %lld doubles",
                            reinterpret_cast<const void*>(client_sqdist_finalize_kernel)};

// the launch step (window.hpp) on a call's workspace: partials[K][parts] (+ extra)
template <class Launch>
int fused_launch(const FusedCall& c, int64_t parts, int64_t extra, Launch&& launch, bool finalize = true) {
  return launch_and_finalize(kRowsLaunch, c.what, c.K, parts, extra, c.partials, c.partial_elems, c.sumsq, c.s, launch,
                             finalize);
}

// Workgroups per CU the fused kernel keeps resident at this K (LDS-bound);
// 0 = the LDS request cannot be granted.
template <int S, bool DB = false, int RW = 0, int RM = 1>
int fused_per_cu(int64_t K) {
  return lds_blocks_per_cu(reduce_sqdist_f32_kernel<S, DB, RW, false, RM>, kBlock, fused_lds_bytes(K, S, DB));
}

template <int S, bool DB = false, int RW = 0, int RM = 1>
int64_t fused_grid(int64_t K, int64_t P, int blocks_per_cu) {
  return persistent_grid(blocks_per_cu > 0 ? blocks_per_cu : fused_per_cu<S, DB, RW, RM>(K), cu_count(),
                         (P + S - 1) / S);
}

// RM = rows per thread in the squares: 1 up to 256 rows, else 2 (the variants')
template <int S, bool DB, int RW, int RM>
int launch_fused_rm(const FusedCall& c, int blocks_per_cu) {
  if (RW > 0 && c.K > 4 * RW)
    return set_error(FEDAVG_EMODE, "%s: %d rows per wave cover K <= %d", c.what, RW, 4 * RW);
  if (fused_per_cu<S, DB, RW, RM>(c.K) <= 0)
    return set_error(FEDAVG_EMODE, "%s: the %d-column tile does not fit LDS at K = %lld", c.what, S, (long long)c.K);
  const int64_t ntiles = (c.P + S - 1) / S;
  const int64_t grid = fused_grid<S, DB, RW, RM>(c.K, c.P, blocks_per_cu);
  return fused_launch(c, grid, 0, [&] {
    hipLaunchKernelGGL((reduce_sqdist_f32_kernel<S, DB, RW, false, RM>), dim3(static_cast<unsigned>(grid)), dim3(kBlock),
                       static_cast<unsigned>(fused_lds_bytes(c.K, S, DB)), c.s, c.clients, static_cast<int>(c.K), c.ld,
                       c.P, ntiles, c.weights, c.out, c.partials);
  });
}

#ifdef FEDAVG_TUNING  // the variants pick RM by K; production names RM 1 (K <= 128)
template <int S, bool DB = false, int RW = 0>
int launch_fused(const FusedCall& c, int blocks_per_cu) {
  if (c.K <= kBlock) return launch_fused_rm<S, DB, RW, 1>(c, blocks_per_cu);
  if constexpr (RW == 0) return launch_fused_rm<S, DB, RW, 2>(c, blocks_per_cu);
  return set_error(FEDAVG_EMODE, "%s: this variant covers K <= %d", c.what, kBlock);
}
#endif  // FEDAVG_TUNING

// ---------------------------------------------------------------------------
// Register-staged fused tiles (round 3).  The LDS-DMA form above fills a
// tile straight into LDS and has nothing in flight while a tile is averaged
// and squared; LDS-DMA also tops out near 6.5-6.8 TB/s chip-wide where
// register loads reach the row reduce's 7.1.  Here the tile goes through
// registers:
//   slot m of thread t holds row r0 + m R, 16-B slice sl of the tile
//   (V = S / 4 slices per row segment, R = 256 / V rows per slot round,
//   r0 = t / V, sl = t % V), so a wave instruction reads 64 / V row segments
//   of S x 4 bytes and the slot's LDS image is the linear 16 (t + 256 m);
// per tile:
//   1. the staged slots (loaded one tile earlier) are written to LDS,
//   2. the NEXT tile's loads are issued into the same registers -- they stay
//      in flight while this tile is averaged and squared,
//   3. the reference's sequential chain, one thread per column (S threads),
//   4. every thread squares its own slots against the tile's average; slot m
//      always belongs to the same row, so one fp64 accumulator per slot lives
//      across all tiles, and the V threads of a row (one per slice) are added
//      in a fixed order at the end: partials[row][workgroup].
// MODE 1 is a traffic probe (loads only: wrong results).
// ---------------------------------------------------------------------------
// FLAGS (probes): 1 = TILED buffer [ntiles][K][S] (each tile's rows contiguous);
// 2 = the workgroups of one XCD take contiguous tiles of a sweep (dispatch
// puts workgroup b on XCD b % 8); 4 = and the workgroups of one CU too
// (b, b + 256, ... share a CU).  Both remaps are bijections of the sweep: a
// different placement only changes the speed.
// DEPTH 2 (64 columns): two tiles' loads in flight per workgroup (two register
// stages, the tile in LDS a third), four waves per SIMD.
template <int S, int SLOTS, int MODE = 0, int FLAGS = 0, int DEPTH = 1>
__global__ __launch_bounds__(kBlock, DEPTH == 1 ? 1 : 4) void reduce_sqdist_rs_kernel(const float* __restrict__ X, int K, int64_t ld,
                                                                  int64_t P, int64_t ntiles,
                                                                  const float* __restrict__ W,
                                                                  float* __restrict__ out,
                                                                  double* __restrict__ partials) {
  static_assert(S == 32 || S == 64 || S == 128 || S == 256, "tile widths: 32, 64, 128 or 256 columns");
  static_assert(DEPTH == 1 || (DEPTH == 2 && S == 64), "one tile in flight, or two of 64 columns");
  constexpr int V = S / 4;
  constexpr int R = kBlock / V;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* gs = lds + K * S;
  const int t = threadIdx.x;
  const int r0 = t / V, sl = t % V;
  const int nslot = r0 < K ? (K - r0 + R - 1) / R : 0;  // slots of this thread that hold a row
  constexpr bool TILED = (FLAGS & 1) != 0;
  const int64_t rstride = TILED ? S : ld;  // TILED: ld unused
  const char* p0 = reinterpret_cast<const char*>(X) + (static_cast<int64_t>(r0) * rstride + 4 * sl) * 4;
  const int64_t mstride = static_cast<int64_t>(R) * rstride * 4;
  f32x4* tile4 = reinterpret_cast<f32x4*>(lds);
  double acc[SLOTS];
#pragma unroll
  for (int m = 0; m < SLOTS; ++m) acc[m] = 0.0;

  // this thread's slots of tile `tt` into registers (slices past the model's
  // end are not loaded: the last row's would run off the allocation)
  const auto issue = [&](f32x4 (&xs)[SLOTS], int64_t tt) {
    const int64_t c0 = tt * S;
    const char* p = p0 + (TILED ? tt * K * S : c0) * 4;
    const bool slice_ok = c0 + 4 * sl < P;
#pragma unroll
    for (int m = 0; m < SLOTS; ++m)
      if (m < nslot && slice_ok) xs[m] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + m * mstride));
  };

  // one tile: staged slots -> LDS, refill the stage with tile `next`, average, squares
  const auto body = [&](f32x4 (&xs)[SLOTS], int64_t tt, int64_t next) {
    const int64_t c0 = tt * S;
    const int ncols = P - c0 < S ? static_cast<int>(P - c0) : S;
    if constexpr (MODE == 1) {
      float probe = 0.f;
#pragma unroll
      for (int m = 0; m < SLOTS; ++m)
        if (m < nslot) probe += xs[m].x;  // consume the loads
      if (next < ntiles) issue(xs, next);
      if (t == 0) out[c0] = probe;
      return;
    }
    barrier_lds();  // every wave is done with the previous tile
#pragma unroll
    for (int m = 0; m < SLOTS; ++m)
      if (m < nslot) tile4[t + kBlock * m] = xs[m];  // 1. (a ragged slice keeps stale data: never used)
    barrier_lds();
    if (next < ntiles) issue(xs, next);  // 2. that stage's next tile in flight
    if (t < S) {  // 3. the average of column t, in the reference's order
      float a = lds[t] * W[0];
      constexpr int kUnroll = S == 64 ? 32 : 16;
#pragma unroll kUnroll
      for (int k = 1; k < K; ++k) {
        const float term = lds[k * S + t] * W[k];
        a = a + term;
      }
      gs[t] = a;
      if (t < ncols) out[c0 + t] = a;
    }
    barrier_lds();
    // 4. squares of this thread's slots: fl32(x - g) as the reference forms it, fp64 square-adds
    const f32x4 g = reinterpret_cast<const f32x4*>(gs)[sl];
    const int nv = ncols - 4 * sl;  // valid columns of this slice
    if (nv >= 4) {
#pragma unroll
      for (int m = 0; m < SLOTS; ++m)
        if (m < nslot) {
          const f32x4 d = tile4[t + kBlock * m] - g;
          const double dx = d.x, dy = d.y, dz = d.z, dw = d.w;
          acc[m] = __builtin_fma(dx, dx, acc[m]);
          acc[m] = __builtin_fma(dy, dy, acc[m]);
          acc[m] = __builtin_fma(dz, dz, acc[m]);
          acc[m] = __builtin_fma(dw, dw, acc[m]);
        }
    } else if (nv > 0) {  // ragged slice: select (not multiply) -- padding may hold NaN/inf
#pragma unroll
      for (int m = 0; m < SLOTS; ++m)
        if (m < nslot) {
          const f32x4 d = tile4[t + kBlock * m] - g;
          const double dx = d.x, dy = nv > 1 ? d.y : 0.f, dz = nv > 2 ? d.z : 0.f;
          acc[m] = __builtin_fma(dx, dx, acc[m]);
          acc[m] = __builtin_fma(dy, dy, acc[m]);
          acc[m] = __builtin_fma(dz, dz, acc[m]);
        }
    }
  };

  int64_t first = blockIdx.x;  // this workgroup's position in every sweep of gridDim.x tiles
  if constexpr ((FLAGS & 6) != 0) {
    const int64_t b = blockIdx.x, per_xcd = gridDim.x / 8;
    if constexpr ((FLAGS & 4) != 0) {
      const int64_t j = b / 8, per_cu = per_xcd / 32;
      first = (b % 8) * per_xcd + (j % 32) * per_cu + j / 32;
    } else {
      first = (b % 8) * per_xcd + b / 8;
    }
  }
  const int64_t G = gridDim.x;
  f32x4 xa[SLOTS];
  if (first < ntiles) issue(xa, first);
  if constexpr (DEPTH == 1) {
    for (int64_t tt = first; tt < ntiles; tt += G) body(xa, tt, tt + G);
  } else {
    f32x4 xb[SLOTS];
    if (first + G < ntiles) issue(xb, first + G);
    for (int64_t tt = first; tt < ntiles; tt += 2 * G) {
      body(xa, tt, tt + 2 * G);
      if (tt + G >= ntiles) break;
      body(xb, tt + G, tt + 3 * G);
    }
  }
  if constexpr (MODE != 0) return;
  // the V slot sums of a row are contiguous in red[]: row * V + slice = t + 256 m
  barrier_loads();
  double* red = reinterpret_cast<double*>(lds);
#pragma unroll
  for (int m = 0; m < SLOTS; ++m)
    if (m < nslot) red[t + kBlock * m] = acc[m];
  barrier_lds();
  for (int row = t; row < K; row += kBlock) {
    double s = red[row * V];
#pragma unroll
    for (int j = 1; j < V; ++j) s += red[row * V + j];
    partials[static_cast<int64_t>(row) * gridDim.x + blockIdx.x] = s;
  }
}

template <int S, int SLOTS, int MODE, int FLAGS = 0, int DEPTH = 1>
int fused_rs_per_cu(int64_t K) {
  return lds_blocks_per_cu(reduce_sqdist_rs_kernel<S, SLOTS, MODE, FLAGS, DEPTH>, kBlock, fused_rs_lds_bytes(K, S));
}

template <int S, int SLOTS, int MODE, int FLAGS = 0, int DEPTH = 1>
int64_t fused_rs_grid(int64_t K, int64_t P, int blocks_per_cu) {
  return persistent_grid(blocks_per_cu > 0 ? blocks_per_cu : fused_rs_per_cu<S, SLOTS, MODE, FLAGS, DEPTH>(K),
                         cu_count(), (P + S - 1) / S);
}

template <int S, int SLOTS, int MODE = 0, int FLAGS = 0, int DEPTH = 1>
int launch_fused_rs(const FusedCall& c, int blocks_per_cu) {
  const int64_t K = c.K;
  if (!fused_rs_slots_cover(K, S, SLOTS))
    return set_error(FEDAVG_EMODE, "%s: %d slots per thread cover K <= %d at %d columns", c.what, SLOTS,
                     SLOTS * 1024 / S, S);
  const int per_cu = fused_rs_per_cu<S, SLOTS, MODE, FLAGS, DEPTH>(K);
  if (per_cu <= 0)
    return set_error(FEDAVG_EMODE, "%s: the %d-column tile does not fit LDS at K = %lld", c.what, S, (long long)K);
  if (blocks_per_cu > per_cu)
    return set_error(FEDAVG_EMODE, "%s: %d workgroups per CU requested, %d resident", c.what, blocks_per_cu, per_cu);
  const int64_t ntiles = (c.P + S - 1) / S;
  const int64_t grid = fused_rs_grid<S, SLOTS, MODE, FLAGS, DEPTH>(K, c.P, blocks_per_cu);
  if ((FLAGS & 6) != 0 && (cu_count() != 256 || grid != (blocks_per_cu > 0 ? blocks_per_cu : per_cu) * 256LL))
    return set_error(FEDAVG_EMODE, "%s: the XCD / CU remaps need a full grid on 256 CUs", c.what);
  return fused_launch(c, grid, 0, [&] {
    hipLaunchKernelGGL((reduce_sqdist_rs_kernel<S, SLOTS, MODE, FLAGS, DEPTH>), dim3(static_cast<unsigned>(grid)),
                       dim3(kBlock), static_cast<unsigned>(fused_rs_lds_bytes(K, S)), c.s, c.clients,
                       static_cast<int>(K), c.ld, c.P, ntiles, c.weights, c.out, c.partials);
  }, MODE == 0);  // the probe modes' partials are not sums
}

// ---------------------------------------------------------------------------
// Wave-owned windows (round 3).  The tile kernels above share a tile between
// the 4 waves of a workgroup: one thread per COLUMN runs the chain from LDS,
// so every tile crosses LDS and a barrier, and each workgroup asks for K row
// segments of only S x 4 bytes at a time.  Here one WAVE owns a window of
// 64 x VEC columns and ALL K rows of it in registers (lane l: columns
// l*VEC .. l*VEC + VEC - 1 of every row; K x VEC VGPRs), so
//   - the chain is per lane, straight from registers (packed fp32 mul/add:
//     the bits of fedavg_reduce_f32), no LDS, no barrier;
//   - the squares are per lane as well, and row i's registers are reloaded
//     with the NEXT window's row i right after row i is squared: the next
//     window's K loads are issued during this window's squares (the
//     hardware's 63-load vmcnt cap throttles the issue, nothing else does),
//     so one register image serves both windows with no double buffer;
//   - a workgroup's NW waves take adjacent windows: NW x 64 x VEC x 4 bytes
//     of every row in flight together (2 KiB at VEC 2, NW 4).
// Row sums: a lane's fp64 partial of row i covers VEC columns; each batch of
// 8 rows is folded across the wave with v_permlane32_swap (8 rows -> 4
// registers, each row over 32 lanes), v_permlane16_swap (-> 2 registers, 16
// lanes per row) and one row_ror:8 exchange (-> 1 register: row 4h + [0, 2,
// 1, 3][l >> 4] in the 8 lanes l with (l >> 3) & 1 = h), added into one fp64
// accumulator per batch that lives across all windows; the 8-lane groups are
// summed once at the end (quad_perm / half-mirror DPP) -> partials[row][wave]
// -> the fixed-order finalize.  Deterministic; windows are read through one
// SGPR buffer descriptor per row whose range ends at the model's last 16-B
// slice (num_records 0 past the last window: the tail's reloads are dropped
// in the address unit, no traffic), columns past P inside the last slice are
// zeroed before the chain.
// MODE 1: loads only (a traffic probe: wrong results).  MODE 4 (probe):
// squares in fp32 (the VEC columns' fl32(d*d) summed in fp32, widened once
// per row): the fp64 VALU stream's share of time and clock, measured.
// ---------------------------------------------------------------------------
// (window helpers: WinVec, fold32/16/8, win_batch_row, win_load, win_sq in common.hpp)

template <int KMAX, int VEC, int NW, int MODE = 0, int MINW = win_min_waves(KMAX, VEC)>
__global__ __launch_bounds__(64 * NW, MINW) void reduce_sqdist_win_kernel(
    const float* __restrict__ X, int K, int64_t ld, int64_t P, int64_t nwin, const float* __restrict__ W,
    float* __restrict__ out, double* __restrict__ partials) {
  typedef typename WinVec<VEC>::T V;
  constexpr int WC = 64 * VEC;
  constexpr int NB = (KMAX + 7) / 8;
  const int lane = threadIdx.x & 63;
  const int64_t GW = static_cast<int64_t>(gridDim.x) * NW;
  const int64_t gw = static_cast<int64_t>(blockIdx.x) * NW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t voff = static_cast<uint32_t>(lane) * VEC * 4;
  const int64_t P4 = (P + 3) & ~static_cast<int64_t>(3);  // rows are read up to their last 16-B slice
  const int64_t row_bytes = ld * 4;
  const bool upper = (lane & 8) != 0;

  // window w's bytes per row (0: no such window -- its loads return 0 and move nothing)
  const auto win_bytes = [&](int64_t w) -> int {
    if (w >= nwin) return 0;
    const int64_t n = P4 - w * WC;
    return static_cast<int>((n < WC ? n : WC) * 4);
  };
  // Rows K..KMAX-1 are padding: loaded through an empty descriptor (0, no
  // traffic) and weighted -0.0 in the chain (x + (+0 * -0) == x for every x,
  // -0 and NaN included); their sums are never written.  Every row bound is
  // computed per window from an opaque copy of K: hoisted out of the window
  // loop the KMAX row masks would not fit the SGPRs.  Row i's descriptor base
  // advances one row per load through an opaque pointer for the same reason.
  // The LDS accumulators are per lane: no other lane touches them, no barrier.
  // LDS: the weights padded to KMAX with -0.0 (read as uniform 16-B
  // broadcasts in the chain), then each wave's per-batch row accumulators
  // [NB][64] (one fp64 per lane per batch: registers are the window's)
  __shared__ __attribute__((aligned(16))) float wl[(KMAX + 3) & ~3];
  __shared__ double accl[NW][NB][64];
  for (int i = threadIdx.x; i < ((KMAX + 3) & ~3); i += 64 * NW) wl[i] = i < K ? W[i] : -0.0f;
  float wv0 = lane < K ? W[lane] : -0.0f, wv1 = 64 + lane < K ? W[64 + lane] : -0.0f;  // LROWS: lane l = W[l], W[64 + l]
  double* acc = &accl[threadIdx.x >> 6][0][lane];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[64 * b] = 0.0;
  __syncthreads();
  // MODE 64 (the 81-100 band's form): rows 0..E-1 of the next window are staged in LDS by
  // LDS-DMA before this window's chain (the VGPR rows free up only in the
  // squares), so E rows stay in flight through the chain; K > E
  constexpr bool LROWS = (MODE & 64) != 0;
  constexpr int E = LROWS ? 24 : 0;
  static_assert(!LROWS || VEC == 2, "LDS rows: 512-B row segments (2 x 64 lanes x 4 B)");
  __shared__ __attribute__((aligned(16))) float rowl[LROWS ? NW : 1][LROWS ? E : 1][LROWS ? WC : 1];
  float* myrows = &rowl[LROWS ? (threadIdx.x >> 6) : 0][0][0];
  // the wave's LDS slot base as a wave-uniform (SGPR) value: M0 for every DMA
  const uint32_t lds_base = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) float*)myrows)));
  const auto dma_row = [&](int i, const char* rp, int bytes) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, bytes, 0x00020000);
    // two dword DMAs of 256 B (all 64 lanes: no exec branch around them)
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(uintptr_t)(lds_base + i * WC * 4), 4, lane * 4, 0, 0, 2);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)(uintptr_t)(lds_base + i * WC * 4 + 256), 4, lane * 4 + 256,
                                             0, 0, 2);
  };
  V x[KMAX];
  {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int nb = win_bytes(gw);
    const char* rp = reinterpret_cast<const char*>(X + gw * WC);
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      if (i < E) {
        asm volatile("" : "+s"(rp));
        dma_row(i, rp, nb);
        rp += row_bytes;
        continue;
      }
      asm volatile("" : "+s"(rp));
      x[i] = win_load<VEC>(__builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, i < Kw ? nb : 0, 0x00020000),
                           voff);
      rp += row_bytes;
    }
  }
  float probe = 0.f;
  for (int64_t w = gw; w < nwin; w += GW) {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int64_t c0 = w * WC;
    const int64_t cl = c0 + lane * VEC;  // this lane's first column
    const int nbn = win_bytes(w + GW);
    const char* rp = reinterpret_cast<const char*>(X + (w + GW) * WC);
    if constexpr (LROWS) {
      // this window's LDS rows have landed (the E oldest loads in flight:
      // at most the KMAX - E VGPR rows issued after them are outstanding)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(KMAX - E < 63 ? KMAX - E : 63) : "memory");  // (2 DMAs per LDS row)
#pragma unroll
      for (int i = 0; i < E; ++i) x[i] = *reinterpret_cast<const V*>(myrows + i * WC + lane * VEC);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // read out before the next window's DMA lands
      const char* rq = reinterpret_cast<const char*>(X + (w + GW) * WC);
#pragma unroll
      for (int i = 0; i < E; ++i) {
        asm volatile("" : "+s"(rq));
        dma_row(i, rq, nbn);
        rq += row_bytes;
      }
      rp += E * row_bytes;  // the VGPR rows start at row E
    }
    const auto reload = [&](int i) {  // row i of the next window into x[i]
      asm volatile("" : "+s"(rp));
      x[i] = win_load<VEC>(__builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, i < Kw ? nbn : 0, 0x00020000),
                           voff);
      rp += row_bytes;
    };
    if constexpr ((MODE & 1) != 0) {
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) probe += x[i][v];
        if (i >= E) reload(i);
      }
      continue;
    }
    const bool ragged = c0 + WC > P;
    if (ragged) {  // columns past P (the last slice's padding) are zeroed: never NaN in the squares
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (cl + v >= P) x[i][v] = 0.f;
      }
    }
    // the reference's chain, per lane: fl32(x_0 w_0), then + fl32(x_i w_i) in client order
    V a;
    if constexpr (LROWS) {
      // weights from VGPR lanes (v_readlane): an LDS read here would wait for
      // the LDS-DMA just issued (the compiler cannot tell the arrays apart)
      asm volatile("" : "+v"(wv0), "+v"(wv1));  // re-read per window: not hoisted into SGPRs
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
        const float wi = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(i < 64 ? wv0 : wv1), i & 63));
        if (i == 0) {
          a = x[0] * wi;
        } else {
          const V t = x[i] * wi;
          a = a + t;
        }
      }
    } else {
    int wo = 0;  // re-read per window (an opaque LDS offset): not held in registers across windows
    asm volatile("" : "+v"(wo));
#pragma unroll
    for (int q = 0; q < (KMAX + 3) / 4; ++q) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(&wl[wo + 4 * q]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = 4 * q + j;
        if (i == 0) {
          a = x[0] * w4[0];
        } else if (i < KMAX) {
          const V t = x[i] * w4[j];
          a = a + t;
        }
      }
    }
    }
    if (!ragged) {
      __builtin_nontemporal_store(static_cast<typename WinVec<VEC>::TA>(a), reinterpret_cast<typename WinVec<VEC>::TA*>(out + cl));
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (cl + v < P) out[cl + v] = a[v];
    }
    // squares of fl32(x - g), each row reloaded with the next window's row as soon as it is squared
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * b + j;
        p[j] = 0.0;
        if (i < KMAX) {
          if constexpr ((MODE & 4) != 0) {  // probe: fp32 squares
            const V d = x[i] - a;
            float sq = d[0] * d[0];
#pragma unroll
            for (int v = 1; v < VEC; ++v) sq = sq + d[v] * d[v];
            p[j] = static_cast<double>(sq);
          } else {
            p[j] = win_sq<VEC>(x[i] - a);
          }
          if (i >= E) reload(i);
        }
      }
      acc[64 * b] += win_fold_batch(p, upper);
    }
  }
  if constexpr ((MODE & 1) != 0) {
    if (probe == 12345.f) out[0] = probe;  // keep the loads
    return;
  }
  const int row_in = win_batch_row(lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double s = win_row_sum(acc[64 * b]);
    const int row = 8 * b + row_in;
    if ((lane & 7) == 0 && row < K) partials[static_cast<int64_t>(row) * GW + gw] = s;
  }
}

// waves of a window launch: every resident workgroup (persistent), or one
// per NW windows when the model has fewer
template <int KMAX, int VEC, int NW, int MODE = 0, int MINW = win_min_waves(KMAX, VEC)>
int64_t fused_win_waves(int64_t P, int blocks_per_cu) {
  const auto kern = reduce_sqdist_win_kernel<KMAX, VEC, NW, MODE, MINW>;
  return window_waves(blocks_per_cu > 0 ? blocks_per_cu : resident_blocks(kern, 64 * NW) / cu_count(), cu_count(),
                      (P + 64 * VEC - 1) / (64 * VEC), NW);
}

template <int KMAX, int VEC, int NW, int MODE = 0, int MINW = win_min_waves(KMAX, VEC)>
int launch_fused_win(const FusedCall& c, int blocks_per_cu) {
  if (c.K > KMAX) return set_error(FEDAVG_EMODE, "%s: this window kernel covers K <= %d", c.what, KMAX);
  if ((MODE & 64) != 0 && c.K <= 24) return set_error(FEDAVG_EMODE, "%s: LDS rows need K > 24", c.what);
  const int64_t waves = fused_win_waves<KMAX, VEC, NW, MODE, MINW>(c.P, blocks_per_cu);
  if (waves <= 0) return set_error(FEDAVG_EMODE, "%s: the window kernel is not resident", c.what);
  const int64_t nwin = (c.P + 64 * VEC - 1) / (64 * VEC);
  return fused_launch(c, waves, 0, [&] {
    hipLaunchKernelGGL((reduce_sqdist_win_kernel<KMAX, VEC, NW, MODE, MINW>), dim3(static_cast<unsigned>(waves / NW)),
                       dim3(64 * NW), 0, c.s, c.clients, static_cast<int>(c.K), c.ld, c.P, nwin, c.weights, c.out,
                       c.partials);
  }, (MODE & 1) == 0);  // MODE 1: loads only
}

// ---------------------------------------------------------------------------
// Split-row windows with point-to-point hand-offs (round 6) for 160-1024 rows
// (fused_plan).  The register-staged tiles ran 500 x 11.2M at 5.4 ms (52 % of
// HBM peak; a tile's K-step chain runs on 32 lanes only).  Here a workgroup of
// ns = ceil(K / 64) <= NSMAX waves owns a window of 64 columns; wave h holds
// rows 64h .. 64h + 63 in registers.  The chain keeps the reference's order:
// it runs wave by wave in row order, each wave handing its fp32 partial over
// LDS to the next, the last one storing the average; then every wave squares
// its rows against the average and reloads them from the next window.  Rows
// past K load through an empty descriptor (+0) with weight -0.0, which leaves
// every chain value unchanged.  The first PF rows of the next window are
// loaded into spare registers as the window starts, so HBM has work while the
// chain runs; after squaring row i < PF the wave takes the prefetched row
// instead of reloading it.  No workgroup barrier anywhere in the window loop
// (round 5's form had one per turn; retired, its figures: profiles/r05/winn/):
//   * wave h > 0 starts its turn when wave h - 1's partial for this window is
//     in LDS (part[h - 1], flag[h - 1] = the window's sequence number), wave
//     ns - 1 publishes the average (avg, flag[NSMAX]); every other wave waits
//     for it before its squares;
//   * a wave's own rows are waited for at its turn (the compiler's vmcnt(PF):
//     the prefetched rows of the next window stay in flight), not at the
//     window's start;
//   * the squares and reloads run at a priority by wave (waves 0-3 first), so
//     the first waves' rows of the next window arrive first and their turns
//     start while the later waves' rows are still streaming.
// The timeline build of the retired barrier form measured its window as chain
// (14.4k cycles with the broadcast weights) + reload phase (9-12k) end to end:
// every turn waited at a barrier for the slowest wave's reloads.
// Hand-off safety: wave h writes part[h] for window s + 1 only after its
// squares of window s, i.e. after the average of s, i.e. after wave h + 1
// read part[h] for s; wave ns - 1 writes avg for s + 1 only after every other
// wave's turn of s + 1, each after its squares of s read avg.  Every wave runs
// the same windows, so every flag a wave waits for is set; the polls are
// bounded (kHandoffSpinMax) so a broken protocol ends in wrong sums (the parity
// tests), never in a hung grid.  Weights by row broadcast (chain8_row_bcast).
// MODE 8 (probe), the timeline build: lane 0 of every wave of the first
// kStampBlocks workgroups stores s_memtime at four points of its first
// kStampWins windows (0 window top, 2 turn starts, 3 partial handed on,
// 4 squared), after the K x G partials (winn_stamp_elems;
// scripts/winn_timeline.py reads them).
// ---------------------------------------------------------------------------
// (kHandoffSpinMax: window.hpp, shared with the zero-copy form)

template <int NSMAX, int PF, int MODE = 0>
__global__ __launch_bounds__(64 * NSMAX, win_min_waves(64, 1)) void reduce_sqdist_winf_kernel(
    const float* __restrict__ X, int K, int64_t ld, int64_t P, int64_t nwin, const float* __restrict__ W,
    float* __restrict__ out, double* __restrict__ partials) {
  constexpr int KH = 64, WC = 64, NB = 8, NWV = 4;
  static_assert(PF >= 1 && PF <= KH, "prefetched rows");
  const int lane = threadIdx.x & 63;
  const int h = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ns = __builtin_amdgcn_readfirstlane(static_cast<int>(blockDim.x >> 6));
  const int r0 = h * KH;
  const int64_t G = gridDim.x;
  const uint32_t voff = static_cast<uint32_t>(lane) * 4;
  const int64_t P4 = (P + 3) & ~static_cast<int64_t>(3);
  const int64_t row_bytes = ld * 4;
  const bool upper = (lane & 8) != 0;
  const auto win_bytes = [&](int64_t w) -> int {
    if (w >= nwin) return 0;
    const int64_t n = P4 - w * WC;
    return static_cast<int>((n < WC ? n : WC) * 4);
  };
  __shared__ double accl[NSMAX][NB][64];
  __shared__ float part[NSMAX][64];
  __shared__ float avg[64];
  __shared__ int flag[NSMAX + 1];
  uint64_t* const stamps = reinterpret_cast<uint64_t*>(partials + static_cast<int64_t>(K) * G);
  int wi = 0;
  const auto stamp = [&](int ph) __attribute__((always_inline)) {
    if constexpr ((MODE & 8) != 0) {
      if (blockIdx.x < kStampBlocks && wi < kStampWins) {
        const uint64_t t = __builtin_amdgcn_s_memtime();
        if (lane == 0) stamps[1 + ((int64_t(blockIdx.x) * NSMAX + h) * kStampWins + wi) * kStampSlots + ph] = t;
      }
    }
  };
  if constexpr ((MODE & 8) != 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) stamps[0] = kStampMagic;
  }
  double* acc = &accl[h][0][lane];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[64 * b] = 0.0;
  if (threadIdx.x <= NSMAX) flag[threadIdx.x] = -1;
  float wv[NWV];  // lane 16r + j of wv[k]: row 16k + j's weight (-0.0 past K)
  handoff_weights(wv, W, r0, lane, K);
  __syncthreads();
  // (handoff_wait / handoff_publish / handoff_weights: window.hpp, one text for both forms)
  const auto wait_flag = [&](int idx, int seq) __attribute__((always_inline)) { handoff_wait(flag, idx, seq); };
  const auto publish = [&](int idx, int seq) __attribute__((always_inline)) { handoff_publish(flag, idx, seq); };
  float x[KH];
  float xp[PF];
  {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int nb = win_bytes(blockIdx.x);
    const char* rp = reinterpret_cast<const char*>(X + static_cast<int64_t>(blockIdx.x) * WC) + r0 * row_bytes;
#pragma unroll
    for (int i = 0; i < KH; ++i) {
      asm volatile("" : "+s"(rp));
      x[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                           __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0,
                                                                             r0 + i < Kw ? nb : 0, 0x00020000),
                                           static_cast<int>(voff), 0, 2));
      rp += row_bytes;
    }
  }
  int seq = 0;
  for (int64_t w = blockIdx.x; w < nwin; w += G, ++seq) {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int64_t c0 = w * WC;
    const int64_t cl = c0 + lane;
    const int nbn = win_bytes(w + G);
    const char* rp = reinterpret_cast<const char*>(X + (w + G) * WC) + r0 * row_bytes;
    stamp(0);
#pragma unroll
    for (int i = 0; i < PF; ++i) {  // the next window's first rows, in flight through the turn
      asm volatile("" : "+s"(rp));
      xp[i] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(
                     __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, r0 + i < Kw ? nbn : 0, 0x00020000),
                     static_cast<int>(voff), 0, 2));
      rp += row_bytes;
    }
    const bool ragged = c0 + WC > P;
    if (ragged) {
#pragma unroll
      for (int i = 0; i < KH; ++i)
        if (cl >= P) x[i] = 0.f;
    }
    // the turn
    float a = -0.0f;  // fl32(-0.0 + p) is p, bit for bit: wave 0 starts the chain from it
    if (h > 0) {
      wait_flag(h - 1, seq);
      a = part[h - 1][lane];
    }
    stamp(2);
    __builtin_amdgcn_s_setprio(3);
    {
      float tc = mul_row_bcast<0>(wv[0], x[0]);
      static_for<KH / 8>([&](auto bc) {
        constexpr int b = decltype(bc)::value;
        constexpr bool last = b == KH / 8 - 1;
        chain8_row_bcast<b % 2, last>(a, tc, wv[b / 2], wv[last ? b / 2 : (b + 1) / 2], x + 8 * b);
      });
    }
    if (h < ns - 1) {
      part[h][lane] = a;
      publish(h, seq);
    } else {
      avg[lane] = a;
      publish(NSMAX, seq);
      if (!ragged) {
        __builtin_nontemporal_store(a, out + cl);
      } else if (cl < P) {
        out[cl] = a;
      }
    }
    stamp(3);
    if (h < ns - 1) {
      __builtin_amdgcn_s_setprio(0);
      wait_flag(NSMAX, seq);
      a = avg[lane];
    }
    // the squares, the next window's rows reloaded behind them: waves 0-3 first
    if (h < 4)
      __builtin_amdgcn_s_setprio(2);
    else if (h < 8)
      __builtin_amdgcn_s_setprio(1);
    else
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * b + j;
        const double d = static_cast<double>(x[i] - a);  // fp32 difference, as the reference forms it
        p[j] = d * d;
        if (i < PF) {
          x[i] = xp[i < PF ? i : 0];
        } else {
          asm volatile("" : "+s"(rp));
          x[i] = __builtin_bit_cast(
              float, __builtin_amdgcn_raw_buffer_load_b32(
                         __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, r0 + i < Kw ? nbn : 0, 0x00020000),
                         static_cast<int>(voff), 0, 2));
          rp += row_bytes;
        }
      }
      acc[64 * b] += win_fold_batch(p, upper);
    }
    __builtin_amdgcn_s_setprio(0);
    stamp(4);
    ++wi;
  }
  const int row_in = win_batch_row(lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double s = win_row_sum(acc[64 * b]);
    const int row = 8 * b + row_in;
    if ((lane & 7) == 0 && r0 + row < K) partials[static_cast<int64_t>(r0 + row) * G + blockIdx.x] = s;
  }
}

// workgroups of the hand-off launch: the resident ones (ceil(K / 64) waves
// each) rounded down to a power of two per CU (split_per_cu), at most one per
// window; 0: none resident
template <int NSMAX, int PF, int MODE = 0>
int64_t fused_winf_grid(int64_t K, int64_t P) {
  const int ns = static_cast<int>((K + 63) / 64);
  return persistent_grid(split_per_cu(resident_blocks(reduce_sqdist_winf_kernel<NSMAX, PF, MODE>, 64 * ns), cu_count()),
                         cu_count(), (P + 63) / 64);
}

template <int NSMAX, int PF, int MODE = 0>
int launch_fused_winf(const FusedCall& c) {
  const int64_t K = c.K;
  if (K > NSMAX * 64 || K < 2)
    return set_error(FEDAVG_EMODE, "%s: these split windows cover 2 <= K <= %d", c.what, NSMAX * 64);
  const int ns = static_cast<int>((K + 63) / 64);
  const int64_t nwin = (c.P + 63) / 64;
  const int64_t grid = fused_winf_grid<NSMAX, PF, MODE>(K, c.P);
  if (grid <= 0) return set_error(FEDAVG_EMODE, "%s: the split window kernel is not resident", c.what);
  return fused_launch(c, grid, (MODE & 8) != 0 ? winn_stamp_elems(NSMAX) : 0, [&] {
    hipLaunchKernelGGL((reduce_sqdist_winf_kernel<NSMAX, PF, MODE>), dim3(static_cast<unsigned>(grid)),
                       dim3(static_cast<unsigned>(64 * ns)), 0, c.s, c.clients, static_cast<int>(K), c.ld, c.P, nwin,
                       c.weights, c.out, c.partials);
  });
}

// (Which one-read kernel serves K rows -- fused_plan, its thresholds, tile tables and LDS sizes, each
// with its measurements: dist_plan.hpp.)

// The production instance a plan names, as a tag: parts(K, P) = workgroups
// (one-wave windows: waves) of its launch, the partials' second dimension;
// launch(call) = that launch.
template <int KMAX, int VEC>
struct WinInstance {  // one-wave windows, 4 waves per workgroup
  static int64_t parts(int64_t, int64_t P) { return fused_win_waves<KMAX, VEC, 4, win_rows_mode(KMAX)>(P, 0); }
  static int launch(const FusedCall& c) { return launch_fused_win<KMAX, VEC, 4, win_rows_mode(KMAX)>(c, 0); }
};
template <int NSMAX, int PF>
struct SplitInstance {  // split-row windows, hand-off form
  static int64_t parts(int64_t K, int64_t P) { return fused_winf_grid<NSMAX, PF>(K, P); }
  static int launch(const FusedCall& c) { return launch_fused_winf<NSMAX, PF>(c); }
};
template <int S>
struct LdsInstance {  // LDS-DMA tiles, K <= 128: one row per thread in the squares (RM 1)
  static int64_t parts(int64_t K, int64_t P) { return fused_grid<S, false, 0, 1>(K, P, 0); }
  static int launch(const FusedCall& c) { return launch_fused_rm<S, false, 0, 1>(c, 0); }
};
template <int S, int SLOTS>
struct RsInstance {  // register-staged tiles
  static int64_t parts(int64_t K, int64_t P) { return fused_rs_grid<S, SLOTS, 0>(K, P, 0); }
  static int launch(const FusedCall& c) { return launch_fused_rs<S, SLOTS>(c, 0); }
};

// f(instance tag) for the production instance plan `pl` names; false: it
// names none.  The only walk over the plan kinds: the workspace size and the
// launch both come through here.
template <class F>
bool with_fused_instance(const FusedPlan& pl, F&& f) {
  switch (pl.kind) {
    case kFusedWin:
      return for_win_band(pl.S, [&](auto kmax, auto vec) { f(WinInstance<decltype(kmax)::value, decltype(vec)::value>{}); });
    case kFusedWinn:
      return for_split(pl.slots,
                       [&](auto nsmax, auto pf) { f(SplitInstance<decltype(nsmax)::value, decltype(pf)::value>{}); });
    case kFusedLds:
      return for_entry<kLdsTiles>(pl.S, kAnyB, [&](auto s, auto) { f(LdsInstance<decltype(s)::value>{}); });
    case kFusedRs:
      return for_entry<kRsTiles>(pl.S, pl.slots,
                                 [&](auto s, auto slots) { f(RsInstance<decltype(s)::value, decltype(slots)::value>{}); });
  }
  return false;
}

// the partials' second dimension of the production launch of plan `pl` on
// this device (0: no instance): the `parts` of fused_plan / fused_workspace
inline int64_t fused_plan_parts(const FusedPlan& pl, int64_t K, int64_t P) {
  int64_t n = 0;
  with_fused_instance(pl, [&](auto inst) { n = decltype(inst)::parts(K, P); });
  return n;
}

inline FusedPlan fused_plan(int64_t K, int64_t P) { return fedavg_impl::fused_plan(K, P, fused_plan_parts); }

// ---------------------------------------------------------------------------
// The distance pass's host side (its plans, forms and workspace sizes:
// dist_plan.hpp).
// ---------------------------------------------------------------------------
// The production form of the fp32 pass on this device: fedavg_client_sqdist_f32
// and fedavg_client_sqdist_workspace both come through here.
template <int U, int C>
int64_t dist_buf_slots() {
  return resident_blocks(client_sqdist_buf_kernel<U, C, 1, dist_chains(C), 0>);
}
PlanEntry dist_plan_here(int64_t P) {
  return dist_plan(P, cu_count(), dist_buf_slots<kDistBufRows, kDistBufCols>(), dist_buf_slots<kDistRows, kDistCols>());
}

// The argument / alignment refusals of every distance entry point, `lanes`
// elements per 16-B slice.
int check_dist(const void* clients, int64_t K, int64_t P, int64_t ld, const void* glob, const double* sumsq, int lanes,
               const char* what) {
  int rc = check_common(clients, K, P, ld, glob, sumsq, what);
  if (rc) return rc;
  if (P == 0) return set_error(FEDAVG_EINVAL, "%s: P must be >= 1", what);
  if (!aligned16(clients) || !aligned16(glob) || (ld % lanes) != 0)
    return set_error(FEDAVG_EALIGN, "%s: needs 16-B aligned clients/glob and ld %% %d == 0", what, lanes);
  return FEDAVG_OK;
}

// One call of the fp32 pass as its launches take it (max_blocks: workgroups
// per launch, 0 = one launch)
struct DistCall {
  const float* clients;
  int64_t K, P, ld;
  const float* glob;
  double* partials;
  int64_t partial_elems;
  double* sumsq;
  int max_blocks;
  hipStream_t s;
  const char* what;
  int64_t nwaves(int cols) const { return dist_waves((P + 3) / 4, cols); }
};

// Equal launches of whole workgroups (round_split); the waves of the launch
// at slice v0 write their partials from wave v0 / span x 4 on.
template <int U, int C, bool BUF = false, int MINW = 1, int ACC = 1, int STYLE = 0>
void launch_sqdist(const DistCall& c) {
  const int64_t nvec = (c.P + 3) / 4;
  constexpr int64_t span = static_cast<int64_t>(kBlock) * C;
  const int64_t blocks = (nvec + span - 1) / span;
  const f32x4* X = reinterpret_cast<const f32x4*>(c.clients);
  const f32x4* Gv = reinterpret_cast<const f32x4*>(c.glob);
  const int K = static_cast<int>(c.K);
  const int64_t nwaves = c.nwaves(C);
  for_each_launch(round_split(nvec, span, c.max_blocks > 0 ? c.max_blocks : blocks), nvec, static_cast<int>(c.P & 3),
                  [&](int64_t v0, int64_t n, int tail, bool, bool) {
                    const dim3 grid(grid_for(n, static_cast<int>(span)));
                    const int64_t wave0 = v0 / span * (kBlock / 64);
                    if constexpr (BUF)
                      hipLaunchKernelGGL((client_sqdist_buf_kernel<U, C, MINW, ACC, STYLE>), grid, dim3(kBlock), 0, c.s,
                                         X + v0, K, c.ld / 4, n, tail, Gv + v0, c.partials, nwaves, wave0);
                    else
                      hipLaunchKernelGGL((client_sqdist_f32x4_kernel<U, C>), grid, dim3(kBlock), 0, c.s, X + v0, K,
                                         c.ld / 4, n, tail, Gv + v0, c.partials, nwaves, wave0);
                  });
}

// the workspace check, `launch` (an int status) and the finalize of a call at `cols` slices per thread
template <class Launch>
int dist_launch(const DistCall& c, int cols, Launch&& launch) {
  return launch_and_finalize(kRowsLaunch, c.what, c.K, c.nwaves(cols), 0, c.partials, c.partials ? c.partial_elems : 0,
                             c.sumsq, c.s, launch);
}

// fedavg_client_sqdist_f32: the plan's entry of kDistBufForms
int sqdist_production(const DistCall& c) {
  const PlanEntry plan = dist_plan_here(c.P);
  return dist_launch(c, plan.b, [&] {
    if (!for_entry<kDistBufForms>(plan.a, plan.b, [&](auto u, auto cols) {
          constexpr int U = decltype(u)::value, C = decltype(cols)::value;
          launch_sqdist<U, C, true, 1, dist_chains(C)>(c);
        }))
      return set_error(FEDAVG_EMODE, "%s: plan U%d x C%d names no kernel instance", c.what, plan.a, plan.b);
    return static_cast<int>(FEDAVG_OK);
  });
}
// One launch of the plan's entry of kDistVecForms + the finalize.
// Rows: [K, ld] with 16-B aligned rows (ld a multiple of the 16-B lane count).
template <class D>
int sqdist_vec_impl(const void* clients, int64_t K, int64_t P, int64_t ld, const void* glob, double* workspace,
                    int64_t workspace_elems, double* sumsq, void* stream, const char* what) {
  constexpr int lanes = D::kLanes;
  if (const int rc = check_dist(clients, K, P, ld, glob, sumsq, lanes, what)) return rc;
  const int64_t nvec = (P + lanes - 1) / lanes;
  const PlanEntry plan = dist_vec_plan(nvec, cu_count());
  const int64_t nwaves = dist_waves(nvec, plan.b);
  hipStream_t s = static_cast<hipStream_t>(stream);
  using vec = typename D::vec;
  return launch_and_finalize(kRowsLaunch, what, K, nwaves, 0, workspace, workspace ? workspace_elems : 0, sumsq, s, [&] {
    if (!for_entry<kDistVecForms>(plan.a, plan.b, [&](auto u, auto cols) {
          constexpr int U = decltype(u)::value, C = decltype(cols)::value;
          hipLaunchKernelGGL((client_sqdist_vec_kernel<D, U, C>), dim3(grid_for(nvec, kBlock * C)), dim3(kBlock), 0, s,
                             reinterpret_cast<const vec*>(clients), static_cast<int>(K), ld / lanes, nvec,
                             static_cast<int>(P % lanes), reinterpret_cast<const vec*>(glob), workspace, nwaves);
        }))
      return set_error(FEDAVG_EMODE, "%s: plan U%d x C%d names no kernel instance", what, plan.a, plan.b);
    return static_cast<int>(FEDAVG_OK);
  });
}

#ifdef FEDAVG_TUNING  // probe library only: the variant codes of include/fedavg_amd_tuning.h
// fedavg_client_sqdist_variant: the global-pointer kernel by unroll x 100 + cols; false: no such code
bool launch_sqdist_variant(int code, const DistCall& c) {
  switch (code) {
    case 404: launch_sqdist<4, 4>(c); return true;
    case 804: launch_sqdist<8, 4>(c); return true;
    case 408: launch_sqdist<4, 8>(c); return true;
    case 208: launch_sqdist<2, 8>(c); return true;
  }
  return false;
}

// fedavg_client_sqdist_buf: the buffer-descriptor kernel by unroll x 100 + cols; false: no such code
bool launch_sqdist_buf_variant(int code, const DistCall& c) {
  switch (code) {
    // production's forms (kDistBufForms): unroll = chains x 10000 + rows per batch
    case 4000216: launch_sqdist<2, 16, true, 1, 4>(c); return true;
    case 4000408: launch_sqdist<4, 8, true, 1, 4>(c); return true;
    case 4000404: launch_sqdist<4, 4, true, 1, 4>(c); return true;
    case 4000802: launch_sqdist<8, 2, true, 1, 2>(c); return true;
    case 408: launch_sqdist<4, 8, true>(c); return true;
    case 804: launch_sqdist<8, 4, true>(c); return true;
    case 216: launch_sqdist<2, 16, true>(c); return true;
    // register-capped forms (launch_bounds min waves per SIMD 3 / 4): more
    // waves resident, fewer loads in flight per wave
    case 30216: launch_sqdist<2, 16, true, 3>(c); return true;
    case 40216: launch_sqdist<2, 16, true, 4>(c); return true;
    case 30408: launch_sqdist<4, 8, true, 3>(c); return true;
    case 116: launch_sqdist<1, 16, true>(c); return true;
    case 112: launch_sqdist<1, 12, true>(c); return true;
    case 212: launch_sqdist<2, 12, true>(c); return true;
    case 208: launch_sqdist<2, 8, true>(c); return true;
    case 808: launch_sqdist<8, 8, true>(c); return true;
    // 2 / 4 interleaved fp64 chains per row (codes + 1,000,000 x ACC)
    case 2000216: launch_sqdist<2, 16, true, 1, 2>(c); return true;
    case 2000408: launch_sqdist<4, 8, true, 1, 2>(c); return true;
    case 8000216: launch_sqdist<2, 16, true, 1, 8>(c); return true;
    case 16000216: launch_sqdist<2, 16, true, 1, 16>(c); return true;
    // U = 0: row k + 1 loads while row k is summed (one row of registers each)
    case 16: launch_sqdist<0, 16, true>(c); return true;
    case 4000016: launch_sqdist<0, 16, true, 1, 4>(c); return true;
    case 4000012: launch_sqdist<0, 12, true, 1, 4>(c); return true;
    case 4000008: launch_sqdist<0, 8, true, 1, 4>(c); return true;
    // 4 chains under a register cap (min waves per SIMD 3 / 4)
    case 4030212: launch_sqdist<2, 12, true, 3, 4>(c); return true;
    case 4030216: launch_sqdist<2, 16, true, 3, 4>(c); return true;
    case 4040208: launch_sqdist<2, 8, true, 4, 4>(c); return true;
    case 4030308: launch_sqdist<3, 8, true, 3, 4>(c); return true;
    // narrow column groups for small models (more workgroups per launch)
    case 4000804: launch_sqdist<8, 4, true, 1, 4>(c); return true;
    case 4000402: launch_sqdist<4, 2, true, 1, 2>(c); return true;
    case 4000801: launch_sqdist<8, 1, true, 1, 1>(c); return true;
    case 4001601: launch_sqdist<16, 1, true, 1, 1>(c); return true;
    case 4000116: launch_sqdist<1, 16, true, 1, 4>(c); return true;
    // interleaved loads and squares, L loads in flight: + 100000000 x L
    case 204000216: launch_sqdist<2, 16, true, 1, 4, 2>(c); return true;
    case 404000216: launch_sqdist<2, 16, true, 1, 4, 4>(c); return true;
    case 804000216: launch_sqdist<2, 16, true, 1, 4, 8>(c); return true;
    case 204000404: launch_sqdist<4, 4, true, 1, 4, 2>(c); return true;
    case 404000404: launch_sqdist<4, 4, true, 1, 4, 4>(c); return true;
    case 204000408: launch_sqdist<4, 8, true, 1, 4, 2>(c); return true;
    case 404000408: launch_sqdist<4, 8, true, 1, 4, 4>(c); return true;
  }
  return false;
}

// a probe entry point's call: `cols_ok` and its refusal, then the code's launch
int sqdist_probe(const DistCall& c, int unroll, int cols, bool cols_ok, const char* cols_list,
                 bool (*launch)(int code, const DistCall&)) {
  if (const int rc = check_dist(c.clients, c.K, c.P, c.ld, c.glob, c.sumsq, 4, c.what)) return rc;
  if (!cols_ok) return set_error(FEDAVG_EMODE, "%s: cols must be %s", c.what, cols_list);
  return dist_launch(c, cols, [&] {
    if (!launch(unroll * 100 + cols, c))
      return set_error(FEDAVG_EMODE, "%s: unsupported unroll=%d cols=%d", c.what, unroll, cols);
    return static_cast<int>(FEDAVG_OK);
  });
}
#endif  // FEDAVG_TUNING

}  // namespace

extern "C" {

int64_t fedavg_client_sqdist_workspace(int64_t K, int64_t P) {
  if (K <= 0 || P <= 0) return 0;
  return dist_workspace(K, P, dist_plan_here(P));
}

int fedavg_client_sqdist_f32(const float* clients, int64_t K, int64_t P, int64_t ld, const float* glob,
                             double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  const char* what = "fedavg_client_sqdist_f32";
  if (const int rc = check_dist(clients, K, P, ld, glob, sumsq, 4, what)) return rc;
  return sqdist_production(
      DistCall{clients, K, P, ld, glob, workspace, workspace_elems, sumsq, 0, static_cast<hipStream_t>(stream), what});
}

int64_t fedavg_client_sqdist_workspace_elems(int64_t K, int64_t P, int64_t elem_size) {
  if (K <= 0 || dist_vec_slices(P, elem_size) <= 0) return 0;
  return dist_vec_workspace(K, P, elem_size, cu_count());
}

int fedavg_client_sqdist_f64(const double* clients, int64_t K, int64_t P, int64_t ld, const double* glob,
                             double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return sqdist_vec_impl<DistF64>(clients, K, P, ld, glob, workspace, workspace_elems, sumsq, stream,
                                  "fedavg_client_sqdist_f64");
}

int fedavg_client_sqdist_f16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld, const uint16_t* glob,
                             double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return sqdist_vec_impl<DistHalf<F16Pk>>(clients, K, P, ld, glob, workspace, workspace_elems, sumsq, stream,
                                          "fedavg_client_sqdist_f16");
}

int fedavg_client_sqdist_bf16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld, const uint16_t* glob,
                              double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return sqdist_vec_impl<DistHalf<BF16Pk>>(clients, K, P, ld, glob, workspace, workspace_elems, sumsq, stream,
                                           "fedavg_client_sqdist_bf16");
}

#ifdef FEDAVG_TUNING  // probe library only (libfedavg_amd_probe.so)
int fedavg_client_sqdist_variant(const float* clients, int64_t K, int64_t P, int64_t ld, const float* glob,
                                 double* workspace, int64_t workspace_elems, double* sumsq, int unroll, int cols,
                                 int max_blocks, void* stream) {
  const DistCall call{clients, K, P, ld, glob, workspace, workspace_elems, sumsq, max_blocks,
                      static_cast<hipStream_t>(stream), "fedavg_client_sqdist_f32"};
  return sqdist_probe(call, unroll, cols, cols == 4 || cols == 8, "4 or 8", launch_sqdist_variant);
}

int fedavg_client_sqdist_buf(const float* clients, int64_t K, int64_t P, int64_t ld, const float* glob,
                             double* workspace, int64_t workspace_elems, double* sumsq, int unroll, int cols,
                             int max_blocks, void* stream) {
  const DistCall call{clients, K, P, ld, glob, workspace, workspace_elems, sumsq, max_blocks,
                      static_cast<hipStream_t>(stream), "fedavg_client_sqdist_buf"};
  return sqdist_probe(call, unroll, cols, cols == 1 || cols == 2 || cols == 4 || cols == 8 || cols == 12 || cols == 16,
                      "1, 2, 4, 8, 12 or 16", launch_sqdist_buf_variant);
}
#endif  // FEDAVG_TUNING

// Aggregate + :291 sums in one pass for K <= kFusedRowsMaxK with 16-B
// aligned rows (fused_plan picks the kernel and tile); otherwise the two
// production passes back to back (fedavg_reduce_f32, then
// fedavg_client_sqdist_f32 on its output).  Either way `out` holds
// fedavg_reduce_f32's bits and sumsq the :291 sums.
int64_t fedavg_reduce_sqdist_workspace(int64_t K, int64_t P) {
  if (K <= 0 || P <= 0) return 0;
  return fused_workspace(K, P, fedavg_client_sqdist_workspace(K, P), fused_plan_parts);
}

int fedavg_reduce_sqdist_f32(const float* clients, int64_t K, int64_t P, int64_t ld, const float* weights, float* out,
                             double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  const char* what = "fedavg_reduce_sqdist_f32";
  int rc = check_common(clients, K, P, ld, weights, out, what);
  if (rc) return rc;
  if (!sumsq || !workspace) return set_error(FEDAVG_EINVAL, "%s: null workspace/sumsq", what);
  // both forms read the rows as 16-B slices (the two-pass fallback's distance
  // pass too): refuse unaligned rows up front rather than after the reduce
  if (!aligned16(clients) || (ld % 4) != 0)
    return set_error(FEDAVG_EALIGN, "%s: needs 16-B aligned rows and ld %% 4 == 0 (reduce alone: fedavg_reduce_f32)",
                     what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P == 0) return zero_sums(kRowsLaunch, what, sumsq, K, s);
  const FusedPlan pl = fused_plan(K, P);
  if (pl.kind != kFusedNone && aligned4(out) && aligned4(weights)) {
    const FusedCall call{clients, K, P, ld, weights, out, workspace, workspace_elems, sumsq, s, what};
    if (!with_fused_instance(pl, [&](auto inst) { rc = decltype(inst)::launch(call); }))
      return set_error(FEDAVG_EMODE, "%s: plan %d / %d / %d names no kernel instance", what, pl.kind, pl.S, pl.slots);
    return rc;
  }
  rc = fedavg_reduce_f32(clients, K, P, ld, weights, out, stream);
  if (rc) return rc;
  return fedavg_client_sqdist_f32(clients, K, P, ld, out, workspace, workspace_elems, sumsq, stream);
}

// the production plan of fedavg_reduce_sqdist_f32 for K x P: kind x
// 1000000 + S x 100 + slots (kind 0 two passes, 1 LDS-DMA tiles, 2
// register-staged tiles, 3 wave-owned windows with S = KMAX, slots = VEC,
// 4 split-row windows with S = rows per wave, slots = most waves per group)
int64_t fedavg_fused_plan_of(int64_t K, int64_t P) {
  const FusedPlan pl = fused_plan(K, P);
  return static_cast<int64_t>(pl.kind) * 1000000 + pl.S * 100 + pl.slots;
}

#ifdef FEDAVG_TUNING  // probe library only (libfedavg_amd_probe.so)
// the fused pass with an explicit tile width (64 / 128 / 256 columns) and
// workgroups per CU (0 = as many as LDS allows); workspace >= K x grid
int fedavg_reduce_sqdist_f32_variant(const float* clients, int64_t K, int64_t P, int64_t ld, const float* weights,
                                     float* out, double* workspace, int64_t workspace_elems, double* sumsq, int cols,
                                     int blocks_per_cu, void* stream) {
  const char* what = "fedavg_reduce_sqdist_f32_variant";
  int rc = check_common(clients, K, P, ld, weights, out, what);
  if (rc) return rc;
  if (P == 0 || K > 1024 || !aligned16(clients) || (ld % 4) != 0 || !sumsq || !workspace)
    return set_error(FEDAVG_EINVAL, "%s: needs 1 <= K <= 1024, P >= 1, 16-B aligned rows", what);
  const FusedCall call{clients, K, P, ld, weights, out, workspace, workspace_elems, sumsq,
                       static_cast<hipStream_t>(stream), what};
  // cols + 1000: double-buffered tiles (the next tile's loads in flight while
  // one is used); + 10000: rows per wave with one register accumulator each
  switch (cols) {
#define FEDAVG_FUSED_CASE(C, DBUF, RWS)                                                                           \
  case C + (DBUF ? 1000 : 0) + (RWS ? 10000 : 0):                                                                \
    return launch_fused<C, DBUF, RWS>(call, blocks_per_cu);
    FEDAVG_FUSED_CASE(64, false, 0)
    FEDAVG_FUSED_CASE(128, false, 0)
    FEDAVG_FUSED_CASE(256, false, 0)
    FEDAVG_FUSED_CASE(64, true, 0)
    FEDAVG_FUSED_CASE(128, true, 0)
    FEDAVG_FUSED_CASE(256, true, 0)
    FEDAVG_FUSED_CASE(64, false, 32)
    FEDAVG_FUSED_CASE(128, false, 32)
    FEDAVG_FUSED_CASE(128, true, 32)
#undef FEDAVG_FUSED_CASE
    // register-staged tiles (reduce_sqdist_rs_kernel): 200000 + S; + 100000:
    // loads only (a traffic probe, wrong results); 310128: the slots of K = 100
    // at 128 columns
    case 200032: return launch_fused_rs<32, 10>(call, blocks_per_cu);
    case 200064: return launch_fused_rs<64, 8>(call, blocks_per_cu);
    case 300064: return launch_fused_rs<64, 8, 1>(call, blocks_per_cu);
    case 310128: return launch_fused_rs<128, 13, 1>(call, blocks_per_cu);
    // + 1000000: the same over a TILED buffer [ceil(P / S)][K][S] (probe: is the
    // row-major tile walk limited by the spread of its K row segments?)
    case 1200064: return launch_fused_rs<64, 8, 0, 1>(call, blocks_per_cu);
    case 1300064: return launch_fused_rs<64, 8, 1, 1>(call, blocks_per_cu);
    case 1310128: return launch_fused_rs<128, 13, 1, 1>(call, blocks_per_cu);
    // + 2000000 / 4000000: XCD-contiguous / XCD- and CU-contiguous tile sweeps
    case 2200064: return launch_fused_rs<64, 8, 0, 2>(call, blocks_per_cu);
    case 2300064: return launch_fused_rs<64, 8, 1, 2>(call, blocks_per_cu);
    case 4200064: return launch_fused_rs<64, 8, 0, 4>(call, blocks_per_cu);
    case 4300064: return launch_fused_rs<64, 8, 1, 4>(call, blocks_per_cu);
    // + 10000000: two tiles in flight per workgroup
    case 10200064: return launch_fused_rs<64, 8, 0, 0, 2>(call, blocks_per_cu);
    // many clients: 16 slots per thread at S = 32 (K <= 512) and S = 64 (K <= 256)
    case 200032 + 1600000: return launch_fused_rs<32, 16>(call, blocks_per_cu);
    case 200064 + 1600000: return launch_fused_rs<64, 16>(call, blocks_per_cu);
    // wave-owned windows (reduce_sqdist_win_kernel): 60000000 + MODE * 1000000
    // + 42 at K <= 100 (4 waves, VEC 2); 70000000 + KMAX * 100 + 40 + VEC
#define FEDAVG_WIN_CASE(MODE)                                                                                     \
  case 60000000 + MODE * 1000000 + 42:                                                                           \
    return launch_fused_win<100, 2, 4, MODE>(call, blocks_per_cu);
    FEDAVG_WIN_CASE(64)  // LDS rows: the 81-100 band's production form
    FEDAVG_WIN_CASE(65)  // LDS rows, loads only (round 6 clock attribution)
    FEDAVG_WIN_CASE(68)  // LDS rows, fp32 squares
#undef FEDAVG_WIN_CASE
#define FEDAVG_WINK_CASE(KMAX, VEC, MINW)                                                                         \
  case 70000000 + KMAX * 100 + 40 + VEC:                                                                         \
    return launch_fused_win<KMAX, VEC, 4, 0, MINW>(call, blocks_per_cu);
    FEDAVG_WINK_CASE(100, 2, 2)
    FEDAVG_WINK_CASE(80, 2, 2)
    FEDAVG_WINK_CASE(64, 2, 3)
    FEDAVG_WINK_CASE(32, 4, 3)
    FEDAVG_WINK_CASE(48, 4, 2)
    FEDAVG_WINK_CASE(16, 4, 4)
    FEDAVG_WINK_CASE(128, 1, 2)
#undef FEDAVG_WINK_CASE
    // split-row windows with point-to-point hand-offs (reduce_sqdist_winf_kernel):
    // 91000000 + MODE * 10000 + PF * 100 + NSMAX (MODE 8: the timeline build)
#define FEDAVG_WINF_CASE(NSMAX, PF, MODE)                                                                        \
  case 91000000 + MODE * 10000 + PF * 100 + NSMAX:                                                              \
    return launch_fused_winf<NSMAX, PF, MODE>(call);
    FEDAVG_WINF_CASE(8, 8, 0)
    FEDAVG_WINF_CASE(8, 16, 0)
    FEDAVG_WINF_CASE(16, 8, 0)
    FEDAVG_WINF_CASE(16, 16, 0)
    FEDAVG_WINF_CASE(16, 16, 8)
#undef FEDAVG_WINF_CASE
    default: return set_error(FEDAVG_EMODE, "%s: %d is no variant code (include/fedavg_amd_tuning.h lists them)", what, cols);
  }
}
#endif  // FEDAVG_TUNING

}  // extern "C"
