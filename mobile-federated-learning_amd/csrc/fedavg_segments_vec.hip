// fedavg_segments_vec.hip -- libfedavg_amd_segvec.so (include/
// fedavg_amd_segvec.h): the fp64 / fp16 / bf16 group of a device-resident
// round reduced straight from the clients' own tensors -- the aggregate
// (:450-457) and the :291 sums of squares in ONE read, no packed rows.
//
// fedavg_fused_vec.hip's one-wave window (reduce_sqdist_vecwin_kernel: the
// dtype rules, the register window, the bit-exact chain) over
// fedavg_segments.hip's key / pointer tables (reduce_sqdist_segwin_kernel's
// pointer form: the forward key scan, one vector load of client addresses per
// 64 clients read back by v_readlane).  The rules and the band tables are
// shared (fused_vec_rules.hpp); the host staging is staging.hpp's
// stage_device_round_vec, fuzzed under sanitizers by tests/native.
#include "fused_vec_rules.hpp"

#include "fedavg_amd_segvec.h"
#include "staging.hpp"

namespace {
using fedavg_staging::SegKey;

thread_local fedavg_impl::ErrorState g_sv_err;

int sv_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_sv_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

int sv_launch_status(const char* what) { return fedavg_impl::launch_status(g_sv_err, what); }

// client addresses arrive as integers: an explicit global pointer, or the
// table loads would be flat loads (fedavg_segments.hip's gptr)
typedef __attribute__((address_space(1))) const int64_t* sv_gptr;

// ---------------------------------------------------------------------------
// The kernel.  keys / ptrs: stage_device_round_vec's tables with the key
// table's units = windows of WC = 64 x SB / sizeof(elem) columns of ONE key
// (lane l: bytes l * SB .. l * SB + SB - 1 of every client's window).
//
// A wave holds one window of all K clients in registers, runs the dtype
// rule's chain per lane (first / step / finish: the bits of
// fedavg_reduce_{f64,f16,bf16} on packed rows), stores the average at
// out + key.out_offset + c0, squares each row against it (sq_add) and reloads
// that row's registers with the wave's NEXT window -- of this key or a later
// one, found by a forward scalar scan of the key table (a wave's windows only
// move forward) -- as soon as the row is squared.  8 rows' per-lane fp64
// partials are folded across the wave at a time (window.hpp) into one
// accumulator per batch that lives across the wave's windows; at the end
// partials[row][wave], then a fixed-order sum per row.  No atomics.
//
// Loads: every row of every window, full or ragged, goes through one
// range-checked buffer descriptor -- base: the client's address of the key +
// the window's first byte; records: the bytes from there to the key's last
// 16-B slice that holds an element (at most the window's 64 x SB), 0 for rows
// >= K and when the wave has no next window.  Sources are 16-B aligned (the
// host refuses others), so a lane's SB-byte load lies wholly inside or wholly
// outside the range: nothing past a key's last 16-B slice is read, and what
// is outside reads 0.  The elements >= numel inside that last slice are
// selected away (T::keep) before the chain and in the average, so padding --
// NaN or inf included -- reaches neither `out` nor a sum.  Rows K .. KMAX-1
// read as zeros and are weighted pad_weight() = -0.0 (acc + 0 * -0.0 == acc).
//
// Stores: keys lie back to back in `out`, so a key starts at any element.
//   - a full window of a key whose first element's address in `out` is a
//     multiple of SB (every window of the key is then: windows are 64 x SB
//     bytes apart) takes one SB-byte vector store per lane;
//   - every other window -- a key's ragged last window, and ALL windows of a
//     key whose output address is not SB-aligned (for instance a bf16 key
//     after a key of an odd number of elements: 2 bytes off a dword) -- takes
//     element stores guarded by column < numel.
// ---------------------------------------------------------------------------
template <class T, int KMAX, int SB, int NW, int MINW = fv_min_waves(KMAX, SB)>
__global__ __launch_bounds__(64 * NW, MINW) void reduce_sqdist_segvecwin_kernel(
    const SegKey* __restrict__ keys, const int64_t* __restrict__ ptrs, int64_t n_keys, int64_t units, int K,
    const typename T::wt* __restrict__ W, typename T::elem* __restrict__ out, double* __restrict__ partials) {
  using unit = typename T::unit;
  using wt = typename T::wt;
  using elem = typename T::elem;
  typedef FvSlice<T, SB> S;
  constexpr int ES = sizeof(elem);
  constexpr int NU = SB / sizeof(unit);
  constexpr int LE = SB / ES;  // elements a lane holds of a client's window
  constexpr int WB = 64 * SB;  // window bytes of a client
  constexpr int WC = 64 * LE;  // window columns
  constexpr int NB = (KMAX + 7) / 8;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t GW = static_cast<int64_t>(gridDim.x) * NW;
  const int64_t gw = static_cast<int64_t>(blockIdx.x) * NW + wv;
  const uint32_t voff = static_cast<uint32_t>(lane) * SB;
  const bool upper = (lane & 8) != 0;

  // LDS: the weights padded to KMAX with -0.0, then each wave's per-batch row
  // accumulators [NB][64] (one fp64 per lane per batch, touched by that lane
  // only: the registers are the window's)
  __shared__ __attribute__((aligned(16))) wt wl[(KMAX + 3) & ~3];
  __shared__ double accl[NW][NB][64];
  for (int i = threadIdx.x; i < ((KMAX + 3) & ~3); i += 64 * NW) wl[i] = i < K ? W[i] : T::pad_weight();
  double* acc = &accl[wv][0][lane];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[64 * b] = 0.0;
  __syncthreads();

  S x[KMAX];
  // A window's K client addresses: one vector load per 64 clients (lane l:
  // clients l and 64 + l; the table is padded so both load unconditionally),
  // issued before the chain that precedes their use; row i reads its address
  // with v_readlane where it is used (an SGPR pair: the descriptor stays
  // uniform, and the KMAX addresses never sit in SGPRs at once)
  int64_t pv[2];
  const auto load_ptrs = [&](const int64_t* P) __attribute__((always_inline)) {
    const sv_gptr q = (sv_gptr)(reinterpret_cast<uintptr_t>(P));
    pv[0] = q[lane];
    if constexpr (KMAX > 64) pv[1] = q[64 + lane];
  };
  const auto ptr_of = [&](int i) __attribute__((always_inline)) {
    const int64_t v = pv[i >> 6];
    int li = i & 63;
    asm volatile("" : "+s"(li));
    const uint32_t lo = __builtin_amdgcn_readlane(static_cast<uint32_t>(v), li);
    const uint32_t hi = __builtin_amdgcn_readlane(static_cast<uint32_t>(static_cast<uint64_t>(v) >> 32), li);
    return reinterpret_cast<const char*>((static_cast<uint64_t>(hi) << 32) | lo);
  };
  // row i of the window that starts `b0` bytes into its key and has `nb`
  // bytes in range (Kw: K, or 0 when there is no such window)
  const auto load_row = [&](int i, int64_t b0, int nb, int Kw) __attribute__((always_inline)) {
    x[i] = fv_load<T, SB>(
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ptr_of(i) + b0), 0, i < Kw ? nb : 0, 0x00020000), voff);
  };

  // window / key indices in 32 bits (the host keeps units < 2^31): uniform
  // values stay on the scalar unit
  const int units32 = static_cast<int>(units), nkeys32 = static_cast<int>(n_keys);
  const int GW32 = static_cast<int>(GW);
  // bytes in range of window `w` of a key of `numel` elements: up to the
  // key's last 16-B slice (w is a window of the key: at least one)
  const auto bytes_of = [&](int64_t numel, int w) __attribute__((always_inline)) {
    const int64_t left = ((numel * ES + 15) & ~static_cast<int64_t>(15)) - static_cast<int64_t>(w) * WB;
    return (left >> 31) != 0 ? WB : (static_cast<int>(left) < WB ? static_cast<int>(left) : WB);
  };
  // valid columns of that window
  const auto cols_of = [&](int64_t numel, int w) __attribute__((always_inline)) {
    const int64_t left = numel - static_cast<int64_t>(w) * WC;
    return (left >> 31) != 0 ? WC : (static_cast<int>(left) < WC ? static_cast<int>(left) : WC);
  };

  int u = static_cast<int>(gw), j = 0, n = 0;
  int64_t c0 = 0, out_off = 0;
  if (u < units32) {
    // the key owning window u (keys without windows share their successor's
    // start and lose the tie): a wave-wide search once, forward scans after
    j = __builtin_amdgcn_readfirstlane(static_cast<int>(
        wave_search_last_le([&](int64_t q) { return keys[q].unit_start; }, n_keys, static_cast<int64_t>(u))));
    const SegKey key = keys[j];
    const int w = u - static_cast<int>(key.unit_start);
    c0 = static_cast<int64_t>(w) * WC;
    n = cols_of(key.numel, w);
    out_off = key.out_offset;
    const int nb = bytes_of(key.numel, w);
    int Kw = K;
    asm volatile("" : "+s"(Kw));
    load_ptrs(ptrs + static_cast<int64_t>(j) * K);
#pragma unroll
    for (int i = 0; i < KMAX; ++i) load_row(i, static_cast<int64_t>(w) * WB, nb, Kw);
  }
  for (; u < units32; u += GW32) {
    // the wave's next window: its key by a forward scan
    const int un = u + GW32;
    int jn = j, nn = 0, nbn = 0;
    int64_t c0n = 0, b0n = 0, out_offn = 0;
    if (un < units32) {
      while (jn + 1 < nkeys32 && static_cast<int>(keys[jn + 1].unit_start) <= un) ++jn;
      const SegKey kn = keys[jn];
      const int w = un - static_cast<int>(kn.unit_start);
      c0n = static_cast<int64_t>(w) * WC;
      b0n = static_cast<int64_t>(w) * WB;
      nn = cols_of(kn.numel, w);
      nbn = bytes_of(kn.numel, w);
      out_offn = kn.out_offset;
    }
    int Kwn = un < units32 ? K : 0;
    asm volatile("" : "+s"(Kwn));
    // the next window's addresses, before the chain (no next window: key j's
    // again, read by no load -- Kwn is 0)
    load_ptrs(ptrs + static_cast<int64_t>(jn) * K);

    const int cl = lane * LE;  // this lane's first column of the window
    const bool ragged = n != WC;
    int nv[NU];  // valid elements of this lane's units (ragged windows only)
    if (ragged) {
#pragma unroll
      for (int q = 0; q < NU; ++q) {
        const int m = n - (cl + q * T::kUnitElems);
        nv[q] = m <= 0 ? 0 : (m < T::kUnitElems ? m : T::kUnitElems);
      }
#pragma unroll
      for (int i = 0; i < KMAX; ++i) {
#pragma unroll
        for (int q = 0; q < NU; ++q) x[i].u[q] = T::keep(x[i].u[q], nv[q]);
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
      for (int q = 0; q < NU; ++q) {
        fv_pin(x[i].u[q]);
        a[q] = i == 0 ? T::first(x[0].u[q], wi) : T::step(a[q], x[i].u[q], wi);
      }
    }
    S g;
#pragma unroll
    for (int q = 0; q < NU; ++q) g.u[q] = T::finish(a[q]);
    elem* o = out + out_off + c0 + cl;
    // uniform: the window's first output address (lanes are SB bytes apart)
    const bool vec_store = !ragged && ((reinterpret_cast<uintptr_t>(out + out_off + c0)) & (SB - 1)) == 0;
    if (vec_store) {
      typename WinVec<SB / 4>::T gv;
      __builtin_memcpy(&gv, &g, SB);
      *reinterpret_cast<typename WinVec<SB / 4>::T*>(o) = gv;
    } else {
      if (ragged) {
#pragma unroll
        for (int q = 0; q < NU; ++q) g.u[q] = T::keep(g.u[q], nv[q]);  // padding: 0 - 0 in the squares
      }
      elem e[LE];
      __builtin_memcpy(e, &g, SB);
#pragma unroll
      for (int v = 0; v < LE; ++v)
        if (cl + v < n) o[v] = e[v];
    }
    // squares of the rounded differences, each row reloaded with the next window's row as soon as it is squared
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      double p[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int i = 8 * b + r;
        p[r] = 0.0;
        if (i < KMAX) {
          double s = 0.0;
#pragma unroll
          for (int q = 0; q < NU; ++q) {
            fv_pin(x[i].u[q]);
            s = T::sq_add(s, x[i].u[q], g.u[q]);
          }
          p[r] = s;
          load_row(i, b0n, nbn, Kwn);
        }
      }
      acc[64 * b] += win_fold_batch(p, upper);
    }
    j = jn;
    c0 = c0n;
    n = nn;
    out_off = out_offn;
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
// workgroup per client): fusedvec_finalize_kernel's scheme, here because a
// kernel launches from its own library only
__global__ __launch_bounds__(kBlock) void segvec_finalize_kernel(const double* __restrict__ partials, int64_t nwaves,
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

// ---------------------------------------------------------------------------
// Host.  The bands are fused_vec_rules.hpp's (kVecBands16 / kVecBands64): one
// instance per band and dtype, grids sized for the constant 256 CUs.
// ---------------------------------------------------------------------------
const PlanEntry* sv_band(int64_t K, int64_t elem_size) {
  return elem_size == 8 ? vec_band_of<kVecBands64>(K) : (elem_size == 2 ? vec_band_of<kVecBands16>(K) : nullptr);
}

const LaunchCtx kSegVecLaunch{sv_error, sv_launch_status, "%s: partials need %lld doubles",
                              reinterpret_cast<const void*>(segvec_finalize_kernel)};

template <class T, auto& Bands>
int device_round_vec(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index, const int64_t* key_numel,
                     const int64_t* key_offset, int64_t n_keys, int64_t K, const double* weights, void* out,
                     double* partials, int64_t partial_elems, double* sumsq, void* host_ws, void* dev_ws,
                     int64_t ws_bytes, void* stream, const char* what) {
  using elem = typename T::elem;
  constexpr int64_t ES = sizeof(elem);
  if (K <= 0 || K > INT32_MAX || n_keys <= 0 || n_keys >= (int64_t(1) << 31))
    return sv_error(FEDAVG_EINVAL, "%s: K and n_keys must be >= 1 (got %lld, %lld)", what, (long long)K,
                    (long long)n_keys);
  if (!client_ptrs || !key_numel || !key_offset || !weights || !out || !partials || !sumsq || !host_ws || !dev_ws)
    return sv_error(FEDAVG_EINVAL, "%s: null argument", what);
  if (!key_index && ptr_ld < n_keys) return sv_error(FEDAVG_EINVAL, "%s: ptr_ld (%lld) < n_keys", what, (long long)ptr_ld);
  const PlanEntry* band = sv_band(K, ES);
  if (!band)
    return sv_error(FEDAVG_EMODE, "%s: %lld clients are beyond the one-wave bands (pack rows instead)", what,
                    (long long)K);
  const fedavg_staging::VecWs L = fedavg_staging::round_vec_ws(K, n_keys);
  if (ws_bytes < L.end) return sv_error(FEDAVG_EINVAL, "%s: workspace needs %lld bytes", what, (long long)L.end);
  if (!aligned16(host_ws) || !aligned16(dev_ws))
    return sv_error(FEDAVG_EALIGN, "%s: workspaces must be 16-B aligned", what);
  // everything the host writes before the tables' H2D, with the sources'
  // null / alignment refusals (staging.hpp)
  const int64_t span = 64 * band->b / ES;
  const fedavg_staging::RoundVecIn rin{client_ptrs, ptr_ld, key_index, key_numel, key_offset, n_keys, K, weights, ES, span};
  fedavg_staging::RoundVecOut st;
  fedavg_staging::Msg msg;
  if (const int rc = fedavg_staging::stage_device_round_vec(rin, host_ws, ws_bytes, &st, &msg))
    return sv_error(rc, "%s: %s", what, msg.text);
  const int64_t waves = window_waves(fv_min_waves(band->a, band->b), kVecCUs, st.units, kVecNW);
  if (partial_elems < K * waves)
    return sv_error(FEDAVG_EINVAL, kSegVecLaunch.too_small, what, (long long)(K * waves));
  if (!is_pinned_host_memory(host_ws)) return sv_error(FEDAVG_EINVAL, "%s: host_ws is not pinned host memory", what);
  if (!is_device_memory(dev_ws) || !is_device_memory(out) || !is_device_memory(sumsq) || !is_device_memory(partials))
    return sv_error(FEDAVG_EINVAL, "%s: dev_ws, out, partials and sumsq must be device memory", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (!st.first_src) {  // every key empty: nothing to read, nothing to average
    const hipError_t e = hipMemsetAsync(sumsq, 0, static_cast<size_t>(K) * sizeof(double), s);
    if (e != hipSuccess) return sv_error(-static_cast<int>(e), "%s: hipMemsetAsync failed", what);
    g_sv_err.clear();
    return FEDAVG_OK;
  }
  // a host address would fault the kernel: spot check of the first and last
  // source (the Python layer checks every tensor's device)
  if (!is_device_memory(st.first_src) || !is_device_memory(st.last_src))
    return sv_error(FEDAVG_EINVAL, "%s: client sources must be device memory", what);
  const hipError_t e = hipMemcpyAsync(dev_ws, host_ws, static_cast<size_t>(st.bytes), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return sv_error(-static_cast<int>(e), "%s: hipMemcpyAsync failed: %s", what, hipGetErrorString(e));
  }
  const char* db = static_cast<const char*>(dev_ws);
  const auto* keys = reinterpret_cast<const SegKey*>(db);
  const auto* tptrs = reinterpret_cast<const int64_t*>(db + L.ptrs);
  const auto* dw = reinterpret_cast<const typename T::wt*>(db + L.w);
  const int64_t units = st.units;
  int rc = FEDAVG_OK;
  const bool found = for_entry<Bands>(band->a, band->b, [&](auto kmax, auto sb) {
    rc = launch_and_finalize(kSegVecLaunch, what, K, waves, 0, partials, partial_elems, sumsq, s, [&] {
      hipLaunchKernelGGL((reduce_sqdist_segvecwin_kernel<T, decltype(kmax)::value, decltype(sb)::value, kVecNW>),
                         dim3(static_cast<unsigned>(waves / kVecNW)), dim3(64 * kVecNW), 0, s, keys, tptrs, n_keys, units,
                         static_cast<int>(K), dw, static_cast<elem*>(out), partials);
    });
  });
  if (!found) return sv_error(FEDAVG_EMODE, "%s: band %d / %d names no kernel instance", what, band->a, band->b);
  return rc;
}

}  // namespace

extern "C" {

int fedavg_segvec_abi_version(void) { return 1; }

const char* fedavg_segvec_last_error(void) { return g_sv_err.c_str(); }

int64_t fedavg_device_round_vec_workspace(int64_t K, int64_t n_keys) {
  return fedavg_staging::round_vec_workspace_bytes(K, n_keys);
}

// K x the waves of the largest grid any instance launches (4 workgroups of 4
// waves on each of 256 CUs): monotone in K, and enough for every band
int64_t fedavg_device_round_vec_partials(int64_t K, int64_t elem_size) {
  if (K <= 0 || (elem_size != 2 && elem_size != 8)) return 0;
  return K * kVecMaxWaves;
}

int64_t fedavg_device_round_vec_plan_of(int64_t K, int64_t elem_size, int is_bf16) {
  (void)is_bf16;  // fp16 and bf16 share their bands
  const PlanEntry* band = sv_band(K, elem_size);
  return band ? 3000000 + static_cast<int64_t>(band->a) * 100 + band->b : 0;
}

int fedavg_device_round_f64(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                            const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys, int64_t K,
                            const double* weights, double* out, double* partials, int64_t partial_elems, double* sumsq,
                            void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return device_round_vec<FvF64, kVecBands64>(client_ptrs, ptr_ld, key_index, key_numel, key_offset, n_keys, K, weights,
                                              out, partials, partial_elems, sumsq, host_ws, dev_ws, ws_bytes, stream,
                                              "fedavg_device_round_f64");
}

int fedavg_device_round_f16(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                            const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys, int64_t K,
                            const double* weights, uint16_t* out, double* partials, int64_t partial_elems,
                            double* sumsq, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return device_round_vec<FvHalf<F16Pk>, kVecBands16>(client_ptrs, ptr_ld, key_index, key_numel, key_offset, n_keys, K,
                                                      weights, out, partials, partial_elems, sumsq, host_ws, dev_ws,
                                                      ws_bytes, stream, "fedavg_device_round_f16");
}

int fedavg_device_round_bf16(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                             const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys, int64_t K,
                             const double* weights, uint16_t* out, double* partials, int64_t partial_elems,
                             double* sumsq, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream) {
  return device_round_vec<FvHalf<BF16Pk>, kVecBands16>(client_ptrs, ptr_ld, key_index, key_numel, key_offset, n_keys, K,
                                                       weights, out, partials, partial_elems, sumsq, host_ws, dev_ws,
                                                       ws_bytes, stream, "fedavg_device_round_bf16");
}

}  // extern "C"
