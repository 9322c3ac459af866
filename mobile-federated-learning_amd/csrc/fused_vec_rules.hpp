// fused_vec_rules.hpp -- the dtype rules of the one-read aggregate + :291
// window kernels for fp64 / fp16 / bf16: fedavg_fused_vec.hip ([K, ld] rows)
// and fedavg_segments_vec.hip (zero-copy, the clients' own tensors).
//
// Everything here stays in an unnamed namespace: each translation unit gets
// its own copy (a kernel launches from its own library only), and the
// kernels' mangled names keep `(anonymous namespace)::FvF64` /
// `FvHalf<...>` as their template arguments (tests/fusedvec_kernels.txt).
#pragma once

#include "window.hpp"

namespace {
using namespace fedavg_impl;

// ---------------------------------------------------------------------------
// Dtype rules over a `unit`: what one register (pair) of a lane's slice holds.
// ---------------------------------------------------------------------------
// fp16 / bf16: a 32-bit word of two elements; R = F16Pk / BF16Pk (common.hpp)
template <class R>
struct FvHalf {
  typedef unsigned int unit;
  typedef float wt;
  typedef unsigned short elem;
  static constexpr int kUnitElems = 2;
  __device__ static wt pad_weight() { return -0.0f; }
  __device__ static unit zero() { return 0u; }
  __device__ static unit first(unit x, wt w) {
    const f32x2 w2{w, w};
    return R::pack(opaque2(R::unpack(x) * w2));  // rh(f32(x) * w)
  }
  __device__ static unit step(unit a, unit x, wt w) {
    const f32x2 w2{w, w};
    const unit t = R::pack(opaque2(R::unpack(x) * w2));     // rh(f32(x) * w)
    return R::pack(opaque2(R::unpack(a) + R::unpack(t)));  // rh(f32(acc) + f32(term))
  }
  __device__ static unit finish(unit a) {
    return static_cast<unit>(R::canon(static_cast<unsigned short>(a & 0xFFFFu))) |
           (static_cast<unit>(R::canon(static_cast<unsigned short>(a >> 16))) << 16);
  }
  // the unit's first n elements, the others zero (select: padding may hold NaN / inf)
  __device__ static unit keep(unit x, int n) { return n >= 2 ? x : (n == 1 ? (x & 0xFFFFu) : 0u); }
  __device__ static double sq_add(double acc, unit x, unit g) {
    // rh(f32(x) - f32(g)), ATen's opmath subtraction rounded to the rows' type, widened exactly
    const f32x2 d = R::unpack(R::pack(opaque2(R::unpack(x) - R::unpack(g))));
    const double a = d.x, b = d.y;
    acc = __builtin_fma(a, a, acc);
    return __builtin_fma(b, b, acc);
  }
};

struct FvF64 {
  typedef double unit;
  typedef double wt;
  typedef double elem;
  static constexpr int kUnitElems = 1;
  __device__ static wt pad_weight() { return -0.0; }
  __device__ static unit zero() { return 0.0; }
  __device__ static unit first(unit x, wt w) { return x * w; }
  __device__ static unit step(unit a, unit x, wt w) {
    const double t = x * w;
    return a + t;
  }
  __device__ static unit finish(unit a) { return a; }
  __device__ static unit keep(unit x, int n) { return n >= 1 ? x : 0.0; }
  __device__ static double sq_add(double acc, unit x, unit g) {
    const double d = x - g;  // fp64 difference, as the reference forms it
    return __builtin_fma(d, d, acc);
  }
};

// A row register pinned in program order (volatile statements keep theirs):
// without it the 16-bit rows' unpacks are scheduled far ahead of their chain
// step or square, two fp32 registers per word for most of the window at once
// -- more than the register file holds
template <class U>
__device__ __forceinline__ void fv_pin(U& v) {
  asm volatile("" : "+v"(v));
}

template <class T, int SB>
struct FvSlice {
  typename T::unit u[SB / sizeof(typename T::unit)];
};

template <class T, int SB>
__device__ __forceinline__ FvSlice<T, SB> fv_load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const typename WinVec<SB / 4>::T v = win_load<SB / 4>(r, off);
  FvSlice<T, SB> s;
  __builtin_memcpy(&s, &v, SB);
  return s;
}

// __launch_bounds__'s second argument, waves per SIMD: the window's KMAX x
// SB / 4 registers and ~40 others within 512 / waves (no instance may spill)
constexpr int fv_min_waves(int kmax, int sb) { return kmax * (sb / 4) <= 64 ? 4 : 3; }

// ---------------------------------------------------------------------------
// Plan (host).  {KMAX, SB} by band, the only place the bands are written:
// KMAX x SB / 4 row registers per lane (64 or 128), so 4 or 3 waves per SIMD.
// ---------------------------------------------------------------------------
constexpr PlanEntry kVecBands16[] = {{16, 16}, {32, 8}, {64, 8}, {100, 4}, {128, 4}};  // fp16 / bf16
constexpr PlanEntry kVecBands64[] = {{16, 16}, {32, 16}, {64, 8}};                      // fp64
constexpr int kVecNW = 4;  // waves per workgroup: adjacent windows, one wave per SIMD
// the chip the grids are sized for (MI355X: 256 CUs); a persistent grid of
// MINW workgroups per CU, never sized by a device query: the workspace
// functions answer without a GPU
constexpr int64_t kVecCUs = 256;
constexpr int64_t kVecMaxWaves = kVecCUs * 4 * kVecNW;  // no instance launches more (MINW <= 4)

template <auto& Bands>
const PlanEntry* vec_band_of(int64_t K) {
  if (K < 1) return nullptr;
  for (const PlanEntry& b : Bands)
    if (K <= b.a) return &b;
  return nullptr;
}

}  // namespace
