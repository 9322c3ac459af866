// window.hpp -- what the window kernels of fedavg_dist.hip ([K, ld] rows) and
// fedavg_segments.hip (zero-copy, device-resident clients) share: the
// register-window helpers, the row-sum folds, the hand-off protocol's wait /
// publish / weights; and, for every fused launcher (fedavg_fused_vec.hip's
// too), the launch-and-finalize step (host).  The band tables, their plan
// dispatch helpers and the grid rules are HIP-free and live in
// plan_table.hpp, included here.
// Everything about where a row comes from stays with the kernels.
#pragma once

#include "common.hpp"
#include "plan_table.hpp"

#include <type_traits>

namespace fedavg_impl {

// ---------------------------------------------------------------------------
// Wave-owned windows (fedavg_dist.hip's reduce_sqdist_win_kernel and
// fedavg_segments.hip's zero-copy form): a wave holds 64 x VEC columns of all
// K rows in registers; each batch of 8 rows' fp64 partials is folded across
// the wave by v_permlane32_swap / v_permlane16_swap / one row_ror:8 exchange
// into one register (8 lanes per row, win_batch_row).
// ---------------------------------------------------------------------------
template <int VEC>
struct WinVec {
  typedef float T __attribute__((ext_vector_type(VEC)));
  // the same vector at dword alignment: window stores into outputs that are
  // only 4-B aligned (a key's offset inside the packed model is any element)
  typedef float TA __attribute__((ext_vector_type(VEC), aligned(4)));
};

// lanes 0-31: a's two halves added (lane l: a[l] + a[l + 32]); lanes 32-63: b's
__device__ __forceinline__ double fold32(double a, double b) {
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const auto lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(ua), static_cast<uint32_t>(ub), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(ua >> 32), static_cast<uint32_t>(ub >> 32),
                                                   false, false);
  const double na = __builtin_bit_cast(double, (static_cast<uint64_t>(hi[0]) << 32) | lo[0]);
  const double nb = __builtin_bit_cast(double, (static_cast<uint64_t>(hi[1]) << 32) | lo[1]);
  return na + nb;
}

// 16-lane rows [a.r0 + a.r1, b.r0 + b.r1, a.r2 + a.r3, b.r2 + b.r3]
__device__ __forceinline__ double fold16(double a, double b) {
  const uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  const auto lo = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(ua), static_cast<uint32_t>(ub), false, false);
  const auto hi = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(ua >> 32), static_cast<uint32_t>(ub >> 32),
                                                   false, false);
  const double na = __builtin_bit_cast(double, (static_cast<uint64_t>(hi[0]) << 32) | lo[0]);
  const double nb = __builtin_bit_cast(double, (static_cast<uint64_t>(hi[1]) << 32) | lo[1]);
  return na + nb;
}

// lanes with bit 3 clear keep a's value + the lane 8 above; set: b's + the lane 8 below
__device__ __forceinline__ double fold8(double a, double b, bool upper) {
  const double send = upper ? a : b;
  const double keep = upper ? b : a;
  return keep + dpp_move_f64<0x128, 0xF>(send);  // row_ror:8 = lane xor 8 within a 16-lane row
}

// batch row held by lane l after fold32 / fold16 / fold8
__device__ __forceinline__ int win_batch_row(int lane) {
  const int r = lane >> 4;
  return 4 * ((lane >> 3) & 1) + (((r & 1) << 1) | (r >> 1));
}

template <int VEC>
__device__ __forceinline__ typename WinVec<VEC>::T win_load(__amdgpu_buffer_rsrc_t r, uint32_t off, uint32_t soff = 0) {
  typedef typename WinVec<VEC>::T V;
  if constexpr (VEC == 1)
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b32(r, static_cast<int>(off), static_cast<int>(soff), 2));
  else if constexpr (VEC == 2)
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b64(r, static_cast<int>(off), static_cast<int>(soff), 2));
  else
    return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(r, static_cast<int>(off), static_cast<int>(soff), 2));
}

template <int VEC>
__device__ __forceinline__ double win_sq(typename WinVec<VEC>::T d) {
  double s = static_cast<double>(d[0]) * static_cast<double>(d[0]);
#pragma unroll
  for (int v = 1; v < VEC; ++v) s = __builtin_fma(static_cast<double>(d[v]), static_cast<double>(d[v]), s);
  return s;
}

// __launch_bounds__'s second argument is waves per SIMD: the window's KMAX x
// VEC registers (+ a quarter more at VEC 1: one square per row per lane
// before the folds) and ~40 others within 512 / waves
constexpr int win_min_waves(int kmax, int vec) {
  const int regs = kmax * vec + (vec == 1 ? kmax / 4 : 0);
  return regs <= 88 ? 4 : (regs <= 128 ? 3 : (regs <= 216 ? 2 : 1));
}

// A batch's 8 rows of per-lane fp64 squares folded into one register (8
// lanes per row, win_batch_row); `upper`: (lane & 8) != 0
__device__ __forceinline__ double win_fold_batch(const double (&p)[8], bool upper) {
  const double q01 = fold32(p[0], p[1]), q23 = fold32(p[2], p[3]);
  const double q45 = fold32(p[4], p[5]), q67 = fold32(p[6], p[7]);
  return fold8(fold16(q01, q23), fold16(q45, q67), upper);
}

// The end of a window kernel: a batch accumulator summed over its row's 8
// lanes (quad_perm / half-mirror DPP); lane 8g of the wave then holds the sum
// of batch row win_batch_row(8g).  (The loop over the batches with its guarded
// store is each kernel's own: as one inlined helper it changed the code of
// every window kernel.)
__device__ __forceinline__ double win_row_sum(double s) {
  s += dpp_move_f64<0xB1, 0xF>(s);   // quad_perm [1,0,3,2]
  s += dpp_move_f64<0x4E, 0xF>(s);   // quad_perm [2,3,0,1]
  s += dpp_move_f64<0x141, 0xF>(s);  // row_half_mirror: the other quad of the 8-lane group
  return s;
}

// ---------------------------------------------------------------------------
// The split-row windows' hand-off protocol (reduce_sqdist_winf_kernel and its
// zero-copy form, reduce_sqdist_segwinf_kernel; the protocol and its safety
// argument: fedavg_dist.hip), the parts that share with unchanged kernel code
// (what does not, with the figures: DESIGN.md section 3).
// ---------------------------------------------------------------------------
// bound on one wait for a flag: x 16 polls of ~100 clocks:
// < 50 ms, a window is ~13 us
constexpr int kHandoffSpinMax = 1 << 16;

// LDS pointers spelled out: a volatile access through a generic pointer is a
// flat_load, whose wait is vmcnt(0) -- every row load of the wave
typedef __attribute__((address_space(3))) volatile int lds_flag_t;

// wait until flag[idx] (LDS) holds `seq`; bounded, so a broken protocol ends
// in wrong sums (the parity tests), never in a hung grid
__device__ __forceinline__ void handoff_wait(int* flag, int idx, int seq) {
  lds_flag_t* f = (lds_flag_t*)&flag[idx];
  // tight polls (no s_sleep): 600 x 10M 4.20 -> 4.09 ms, 1000 x 12.5M 7.97 -> 7.93
  // (profiles/r06/winf_modes/)
  for (int it = 0; __builtin_amdgcn_readfirstlane(*f) != seq && it < kHandoffSpinMax * 16; ++it) {
  }
  asm volatile("" ::: "memory");
}
// flag[idx] = seq once the payload's ds_write is done
__device__ __forceinline__ void handoff_publish(int* flag, int idx, int seq) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  *(lds_flag_t*)&flag[idx] = seq;
}

// the chain's weights by row broadcast: lane 16r + j of wv[k] holds row
// r0 + 16k + j's weight (-0.0 past K)
__device__ __forceinline__ void handoff_weights(float (&wv)[4], const float* W, int r0, int lane, int K) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int row = r0 + 16 * k + (lane & 15);
    wv[k] = row < K ? W[row] : -0.0f;
  }
}

// ---------------------------------------------------------------------------
// The launch step of every fused aggregate + :291 launcher (host; the plan
// tables and grid rules: plan_table.hpp).
// ---------------------------------------------------------------------------
// What a translation unit's launches share: its library's error state, the
// wording of its "too small" refusal (what, doubles needed) and the kernel
// that sums partials[K][parts] into sumsq[K]
struct LaunchCtx {
  int (*error)(int code, const char* fmt, ...);
  int (*status)(const char* what);
  const char* too_small;
  const void* finalize;  // __global__ void(const double* partials, int64_t parts, double* sumsq), kBlock threads
};

// The one launch path: refuse partials of fewer than K x parts + extra
// doubles, issue the main launch (`launch`: void, or an int status that ends
// the call when non-zero), check it, sum the partials (unless `finalize` is
// false: probe modes whose partials are not sums), check that.
template <class Launch>
int launch_and_finalize(const LaunchCtx& cx, const char* what, int64_t K, int64_t parts, int64_t extra,
                        double* partials, int64_t partial_elems, double* sumsq, hipStream_t s, Launch&& launch,
                        bool finalize = true) {
  const int64_t need = K * parts + extra;
  if (partial_elems < need) return cx.error(FEDAVG_EINVAL, cx.too_small, what, (long long)need);
  if constexpr (std::is_void_v<decltype(launch())>) {
    launch();
  } else if (const int rc = launch()) {
    return rc;
  }
  const int rc = cx.status(what);
  if (rc || !finalize) return rc;
  const double* sums_of = partials;
  void* args[] = {&sums_of, &parts, &sumsq};
  (void)hipLaunchKernel(cx.finalize, dim3(static_cast<unsigned>(K)), dim3(kBlock), args, 0, s);
  return cx.status(what);
}

// nothing to read (no columns, no units): every client's sum is 0
inline int zero_sums(const LaunchCtx& cx, const char* what, double* sumsq, int64_t K, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(sumsq, 0, static_cast<size_t>(K) * sizeof(double), s);
  return e == hipSuccess ? FEDAVG_OK : cx.error(-static_cast<int>(e), "%s: hipMemsetAsync failed", what);
}

}  // namespace fedavg_impl
