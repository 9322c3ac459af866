// fedavg_fused_vec.hip -- libfedavg_amd_fusedvec.so (include/
// fedavg_amd_fusedvec.h): the aggregate (:450-457) and the :291 sums of
// squares in ONE read of fp64 / fp16 / bf16 rows.
//
// The fp32 one-wave window (fedavg_dist.hip's reduce_sqdist_win_kernel) over
// a dtype rule: a wave owns a window of 64 lanes x SB bytes of ALL K rows in
// registers (lane l: bytes l*SB .. l*SB + SB - 1 of every row's window), so
//   - the reference's chain runs per lane, straight from registers, with the
//     dtype's own rounding (fp64: multiply, then add; fp16 / bf16: fp32
//     opmath rounded to the storage type after every operation, the packed
//     converts of reduce_vec_kernel<OpHalfPk<..>>): the bits of
//     fedavg_reduce_{f64,f16,bf16};
//   - the average is stored, and every row is squared against it while it is
//     still in registers (the difference rounded as the reference's
//     `w[para] - w_glob[para]`, squares and sums in fp64 by fused
//     multiply-adds); row i's registers are reloaded with the NEXT window's
//     row i as soon as row i is squared, so one register image serves both
//     windows;
//   - each batch of 8 rows' per-lane partials is folded across the wave
//     (window.hpp: win_fold_batch) into one fp64 accumulator per batch that
//     lives across all windows of the wave; at the end partials[row][wave],
//     then a fixed-order sum per row.  No floating-point atomics.
// Rows are read through one buffer descriptor per row and window whose range
// ends at the row's last 16-B slice that holds a column < P (0 bytes for rows
// >= K and windows past the last: nothing is read); the columns >= P of that
// slice are zeroed (selected) before the chain and in the average, so
// padding never reaches a sum.  Rows K .. KMAX-1 read as zeros and are
// weighted -0.0 (acc + (0 * -0.0) == acc for every acc); their sums are
// never written.
#include "fused_vec_rules.hpp"  // the dtype rules, the row slices and the band tables

#include "fedavg_amd_fusedvec.h"

namespace {
using namespace fedavg_impl;

thread_local ErrorState g_fv_err;

int fv_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_fv_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int fv_launch_status(const char* what) { return launch_status(g_fv_err, what); }

// ---------------------------------------------------------------------------
// The kernel.  X: the rows as bytes; row_bytes = ld * sizeof(elem), a multiple
// of 16; nwin = windows of 64 * SB bytes that hold a column < P.
// ---------------------------------------------------------------------------
template <class T, int KMAX, int SB, int NW, int MINW = fv_min_waves(KMAX, SB)>
__global__ __launch_bounds__(64 * NW, MINW) void reduce_sqdist_vecwin_kernel(
    const char* __restrict__ X, int K, int64_t row_bytes, int64_t P, int64_t nwin,
    const typename T::wt* __restrict__ W, typename T::elem* __restrict__ out, double* __restrict__ partials) {
  using unit = typename T::unit;
  using wt = typename T::wt;
  using elem = typename T::elem;
  typedef FvSlice<T, SB> S;
  constexpr int ES = sizeof(elem);
  constexpr int NU = SB / sizeof(unit);
  constexpr int LE = SB / ES;   // elements a lane holds of a row
  constexpr int WB = 64 * SB;   // window bytes of a row
  constexpr int WC = 64 * LE;   // window columns
  constexpr int NB = (KMAX + 7) / 8;
  const int lane = threadIdx.x & 63;
  const int64_t GW = static_cast<int64_t>(gridDim.x) * NW;
  const int64_t gw = static_cast<int64_t>(blockIdx.x) * NW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t voff = static_cast<uint32_t>(lane) * SB;
  const int64_t PB = (P * ES + 15) & ~static_cast<int64_t>(15);  // rows are read up to their last 16-B slice
  const bool upper = (lane & 8) != 0;

  // window w's bytes per row (0: no such window -- its loads return 0 and move nothing)
  const auto win_bytes = [&](int64_t w) -> int {
    if (w >= nwin) return 0;
    const int64_t n = PB - w * WB;
    return static_cast<int>(n < WB ? n : WB);
  };
  // LDS: the weights padded to KMAX with -0.0, then each wave's per-batch row
  // accumulators [NB][64] (one fp64 per lane per batch, touched by that lane
  // only: the registers are the window's)
  __shared__ __attribute__((aligned(16))) wt wl[(KMAX + 3) & ~3];
  __shared__ double accl[NW][NB][64];
  for (int i = threadIdx.x; i < ((KMAX + 3) & ~3); i += 64 * NW) wl[i] = i < K ? W[i] : T::pad_weight();
  double* acc = &accl[threadIdx.x >> 6][0][lane];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[64 * b] = 0.0;
  __syncthreads();

  S x[KMAX];
  {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int nb = win_bytes(gw);
    const char* rp = X + gw * WB;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      asm volatile("" : "+s"(rp));
      x[i] = fv_load<T, SB>(__builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, i < Kw ? nb : 0, 0x00020000),
                            voff);
      rp += row_bytes;
    }
  }
  for (int64_t w = gw; w < nwin; w += GW) {
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    const int64_t c0 = w * WC;
    const int64_t cl = c0 + lane * LE;  // this lane's first column
    const int nbn = win_bytes(w + GW);
    const char* rp = X + (w + GW) * WB;
    const auto reload = [&](int i) {  // row i of the wave's next window into x[i]
      asm volatile("" : "+s"(rp));
      x[i] = fv_load<T, SB>(__builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(rp), 0, i < Kw ? nbn : 0, 0x00020000),
                            voff);
      rp += row_bytes;
    };
    const bool ragged = c0 + WC > P;
    int nv[NU];  // valid elements of this lane's units (ragged windows only)
    if (ragged) {
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        const int64_t n = P - (cl + u * T::kUnitElems);
        nv[u] = n <= 0 ? 0 : (n < T::kUnitElems ? static_cast<int>(n) : T::kUnitElems);
      }
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
#pragma unroll
        for (int u = 0; u < NU; ++u) x[i].u[u] = T::keep(x[i].u[u], nv[u]);
      }
    }
    // the reference's chain, per lane, in client order
    unit a[NU];
    int wo = 0;  // re-read per window (an opaque LDS offset): the weights are not held in registers across windows
    asm volatile("" : "+v"(wo));
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
      const wt wi = wl[wo + i];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        fv_pin(x[i].u[u]);
        a[u] = i == 0 ? T::first(x[0].u[u], wi) : T::step(a[u], x[i].u[u], wi);
      }
    }
    S g;
#pragma unroll
    for (int u = 0; u < NU; ++u) g.u[u] = T::finish(a[u]);
    if (!ragged) {
      typename WinVec<SB / 4>::T gv;
      __builtin_memcpy(&gv, &g, SB);
      *reinterpret_cast<typename WinVec<SB / 4>::T*>(reinterpret_cast<char*>(out) + w * WB + voff) = gv;
    } else {
#pragma unroll
      for (int u = 0; u < NU; ++u) g.u[u] = T::keep(g.u[u], nv[u]);  // padding: 0 - 0 in the squares
      elem e[LE];
      __builtin_memcpy(e, &g, SB);
#pragma unroll
      for (int v = 0; v < LE; ++v)
        if (cl + v < P) out[cl + v] = e[v];
    }
    // squares of the rounded differences, each row reloaded with the next window's row as soon as it is squared
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int i = 8 * b + j;
        p[j] = 0.0;
        if (i < KMAX) {
          double s = 0.0;
#pragma unroll
          for (int u = 0; u < NU; ++u) {
            fv_pin(x[i].u[u]);
            s = T::sq_add(s, x[i].u[u], g.u[u]);
          }
          p[j] = s;
          reload(i);
        }
      }
      acc[64 * b] += win_fold_batch(p, upper);
    }
  }
  const int row_in = win_batch_row(lane);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const double s = win_row_sum(acc[64 * b]);
    const int row = 8 * b + row_in;
    if ((lane & 7) == 0 && row < K) partials[static_cast<int64_t>(row) * GW + gw] = s;
  }
}

// sumsq[k] = the sum over waves of partials[k][*] in a fixed order (a
// workgroup per client): client_sqdist_finalize_kernel's scheme
// (fedavg_dist.hip), here because a kernel launches from its own library only
__global__ __launch_bounds__(kBlock) void fusedvec_finalize_kernel(const double* __restrict__ partials, int64_t nwaves,
                                                                   double* __restrict__ out) {
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

// Plan (host): the band tables are fused_vec_rules.hpp's.
const PlanEntry* vec_band(int64_t K, int64_t P, int64_t elem_size) {
  if (P <= 0) return nullptr;
  return elem_size == 8 ? vec_band_of<kVecBands64>(K) : (elem_size == 2 ? vec_band_of<kVecBands16>(K) : nullptr);
}

// this library's error state behind the shared launch step (window.hpp)
const LaunchCtx kVecLaunch{fv_error, fv_launch_status, "%s: workspace needs %lld doubles",
                           reinterpret_cast<const void*>(fusedvec_finalize_kernel)};

template <class T, int KMAX, int SB>
int launch_vecwin(const void* clients, int64_t K, int64_t P, int64_t ld, const void* weights, void* out,
                  double* workspace, int64_t workspace_elems, double* sumsq, hipStream_t s, const char* what) {
  constexpr int ES = sizeof(typename T::elem);
  const int64_t nwin = (P * ES + 64 * SB - 1) / (64 * SB);
  const int64_t waves = window_waves(fv_min_waves(KMAX, SB), kVecCUs, nwin, kVecNW);  // = partials per row
  return launch_and_finalize(kVecLaunch, what, K, waves, 0, workspace, workspace_elems, sumsq, s, [&] {
    hipLaunchKernelGGL((reduce_sqdist_vecwin_kernel<T, KMAX, SB, kVecNW>), dim3(static_cast<unsigned>(waves / kVecNW)),
                       dim3(64 * kVecNW), 0, s, static_cast<const char*>(clients), static_cast<int>(K), ld * ES, P, nwin,
                       static_cast<const typename T::wt*>(weights), static_cast<typename T::elem*>(out), workspace);
  });
}

// the product library's message behind a failing call of the two-pass route
int fv_product_error(int rc, const char* what) {
  return fv_error(rc, "%s: %s", what, fedavg_last_error());
}

template <class T, auto& Bands, class Reduce, class Sqdist>
int reduce_sqdist_vec(const void* clients, int64_t K, int64_t P, int64_t ld, const void* weights, void* out,
                      double* workspace, int64_t workspace_elems, double* sumsq, void* stream, Reduce reduce,
                      Sqdist sqdist, const char* what) {
  constexpr int64_t ES = sizeof(typename T::elem);
  if (K <= 0) return fv_error(FEDAVG_EINVAL, "%s: K must be >= 1 (got %lld)", what, (long long)K);
  if (K > INT32_MAX) return fv_error(FEDAVG_EINVAL, "%s: K too large", what);
  if (P < 0) return fv_error(FEDAVG_EINVAL, "%s: P must be >= 0", what);
  if (ld < P) return fv_error(FEDAVG_EINVAL, "%s: ld (%lld) < P (%lld)", what, (long long)ld, (long long)P);
  if (P > 0 && (!clients || !weights || !out)) return fv_error(FEDAVG_EINVAL, "%s: null buffer", what);
  if (P > 0 && (!sumsq || !workspace)) return fv_error(FEDAVG_EINVAL, "%s: null workspace/sumsq", what);
  // both routes read the rows as 16-B slices: refuse unaligned rows before any work
  if (P > 0 && (!aligned16(clients) || !aligned16(out) || (ld * ES) % 16 != 0))
    return fv_error(FEDAVG_EALIGN, "%s: needs 16-B aligned rows and out, and ld * %d %% 16 == 0", what, (int)ES);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (P == 0) {
    if (!sumsq) return FEDAVG_OK;  // nothing to reduce, nothing to write
    const hipError_t e = hipMemsetAsync(sumsq, 0, static_cast<size_t>(K) * sizeof(double), s);
    return e == hipSuccess ? FEDAVG_OK : fv_error(-static_cast<int>(e), "%s: hipMemsetAsync failed", what);
  }
  if (const PlanEntry* band = vec_band(K, P, ES)) {
    int rc = FEDAVG_OK;
    const bool found = for_entry<Bands>(band->a, band->b, [&](auto kmax, auto sb) {
      rc = launch_vecwin<T, decltype(kmax)::value, decltype(sb)::value>(clients, K, P, ld, weights, out, workspace,
                                                                         workspace_elems, sumsq, s, what);
    });
    if (!found) return fv_error(FEDAVG_EMODE, "%s: band %d / %d names no kernel instance", what, band->a, band->b);
    return rc;
  }
  int rc = reduce(clients, K, P, ld, weights, out, stream);
  if (rc) return fv_product_error(rc, what);
  rc = sqdist(clients, K, P, ld, out, workspace, workspace_elems, sumsq, stream);
  if (rc) return fv_product_error(rc, what);
  g_fv_err.clear();
  return FEDAVG_OK;
}

}  // namespace

extern "C" {

int fedavg_fusedvec_abi_version(void) { return 1; }

const char* fedavg_fusedvec_last_error(void) { return g_fv_err.c_str(); }

// K x the most partials per row either route writes.  Fused: the finest
// slice's windows (4 B per lane), at most kVecMaxWaves.  Two passes: the
// distance pass's finest grid (workgroups of 256 x 2 slices of 16 B, a wave's
// partial each).  Both grow with P and neither depends on K, so the answer
// is monotone in K and in P, and holds for every K.
int64_t fedavg_reduce_sqdist_vec_workspace(int64_t K, int64_t P, int64_t elem_size) {
  if (K <= 0 || P <= 0 || (elem_size != 2 && elem_size != 8)) return 0;
  const int64_t nwin = (P * elem_size + 255) / 256;
  const int64_t win_waves = (nwin + kVecNW - 1) / kVecNW * kVecNW;
  const int64_t fused = win_waves < kVecMaxWaves ? win_waves : kVecMaxWaves;
  const int64_t nvec = (P * elem_size + 15) / 16;
  const int64_t two_pass = (nvec + kBlock * 2 - 1) / (kBlock * 2) * (kBlock / 64);
  return K * (fused > two_pass ? fused : two_pass);
}

int64_t fedavg_fused_vec_plan_of(int64_t K, int64_t P, int64_t elem_size, int is_bf16) {
  (void)is_bf16;  // fp16 and bf16 share their bands
  const PlanEntry* band = vec_band(K, P, elem_size);
  return band ? 3000000 + static_cast<int64_t>(band->a) * 100 + band->b : 0;
}

int fedavg_reduce_sqdist_f64(const double* clients, int64_t K, int64_t P, int64_t ld, const double* weights,
                             double* out, double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return reduce_sqdist_vec<FvF64, kVecBands64>(
      clients, K, P, ld, weights, out, workspace, workspace_elems, sumsq, stream,
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* w, void* o, void* st) {
        return fedavg_reduce_f64(static_cast<const double*>(c), k, p, l, static_cast<const double*>(w),
                                 static_cast<double*>(o), st);
      },
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* g, double* ws, int64_t n, double* sq, void* st) {
        return fedavg_client_sqdist_f64(static_cast<const double*>(c), k, p, l, static_cast<const double*>(g), ws, n,
                                        sq, st);
      },
      "fedavg_reduce_sqdist_f64");
}

int fedavg_reduce_sqdist_f16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld, const float* weights,
                             uint16_t* out, double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return reduce_sqdist_vec<FvHalf<F16Pk>, kVecBands16>(
      clients, K, P, ld, weights, out, workspace, workspace_elems, sumsq, stream,
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* w, void* o, void* st) {
        return fedavg_reduce_f16(static_cast<const uint16_t*>(c), k, p, l, static_cast<const float*>(w),
                                 static_cast<uint16_t*>(o), st);
      },
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* g, double* ws, int64_t n, double* sq, void* st) {
        return fedavg_client_sqdist_f16(static_cast<const uint16_t*>(c), k, p, l, static_cast<const uint16_t*>(g), ws,
                                        n, sq, st);
      },
      "fedavg_reduce_sqdist_f16");
}

int fedavg_reduce_sqdist_bf16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld, const float* weights,
                              uint16_t* out, double* workspace, int64_t workspace_elems, double* sumsq, void* stream) {
  return reduce_sqdist_vec<FvHalf<BF16Pk>, kVecBands16>(
      clients, K, P, ld, weights, out, workspace, workspace_elems, sumsq, stream,
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* w, void* o, void* st) {
        return fedavg_reduce_bf16(static_cast<const uint16_t*>(c), k, p, l, static_cast<const float*>(w),
                                  static_cast<uint16_t*>(o), st);
      },
      [](const void* c, int64_t k, int64_t p, int64_t l, const void* g, double* ws, int64_t n, double* sq, void* st) {
        return fedavg_client_sqdist_bf16(static_cast<const uint16_t*>(c), k, p, l, static_cast<const uint16_t*>(g),
                                         ws, n, sq, st);
      },
      "fedavg_reduce_sqdist_bf16");
}

}  // extern "C"
