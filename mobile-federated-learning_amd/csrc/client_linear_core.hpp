// client_linear_core.hpp -- the device code the two linear-client units share (fedavg_client_linear.hip: the batch
// of at most 64 samples; fedavg_client_stream.hip: the batch walked in groups of rows): the register layout's
// constants, the matrix instruction, the masked batch accessor, the workgroup sum, one slice through the step of the
// rules headers and one sample's softmax / dz.  A unit includes the rules headers itself and then this file.
#pragma once

#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

constexpr int kLinThreads = 512, kLinWaves = kLinThreads / 64;
constexpr int kLinSlots = 64 / kLinWaves;  // tiles of 16 columns per wave
// kLinMaxB: the rows whose logits the workgroup holds at once
constexpr int kLinMaxB = 64, kLinMaxC = 16, kLinMaxD = 16 * kLinWaves * kLinSlots;
// B * (D4 + 4) floats <= B * D + 7 B: every B * D <= 32 * 1024 with B <= 64 fits
constexpr int64_t kLinResidentBytes = 4 * (32 * 1024 + 7 * kLinMaxB);
static_assert(kLinMaxD == 1024, "the header's range");

// v as a value the compiler cannot follow: what is derived from it inside an epoch is formed there, and not
// once before the loop in registers the parameters need
__device__ __forceinline__ int lin_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The batch as the products read it.  RES: rows of S floats in LDS, columns
// [D, D4) zeroed; else global memory.  Outside the batch: 0, and no access.
template <bool RES>
struct LinBatch {
  const float* xs;
  const float* x;
  int B, D, D4, S;
  // x[b][d .. d + 3], d a multiple of 4
  __device__ __forceinline__ f32x4 row4(int b, int d) const {
    if constexpr (RES) {
      const bool on = b < B && d < D4;
      const f32x4 v = *reinterpret_cast<const f32x4*>(xs + (on ? b * S + d : 0));
      return on ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = at(b, d + r);
      return v;
    }
  }
  __device__ __forceinline__ float at(int b, int d) const {
    if constexpr (RES) {
      const bool on = b < B && d < D4;
      const float v = xs[on ? b * S + d : 0];
      return on ? v : 0.f;
    } else {
      const bool on = b < B && d < D;
      const float v = x[on ? static_cast<int64_t>(b) * D + d : 0];
      return on ? v : 0.f;
    }
  }
};

// v[j] = the workgroup's sum of v[j], the same value in every thread
__device__ __forceinline__ void lin_block_sum(double (&v)[kClientStats], double (*red)[kLinWaves]) {
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kClientStats; ++j) {
    const double s = wave_sum_dpp(v[j]);
    if ((threadIdx.x & 63u) == 0) red[j][threadIdx.x >> 6] = s;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kClientStats; ++j) {
    double t = red[j][0];
#pragma unroll
    for (int w = 1; w < kLinWaves; ++w) t += red[j][w];
    v[j] = t;
  }
}

__device__ __forceinline__ CliSlice lin_slice(const float (&v)[4]) {
  return CliSlice{{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}};
}

__device__ __forceinline__ void lin_unslice(float (&v)[4], const CliSlice& s) {
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = __uint_as_float(s.w[r]);
}

// one slice of four parameters through the step of the rules headers
template <bool ADAM>
__device__ __forceinline__ void lin_step(float (&w)[4], const float (&g)[4], float (&m)[4], float (&v)[4],
                                         float (&vx)[4], float alpha, int form, const AdamCoef<float>& c, int live,
                                         int& nans, double& a_w, double& a_d) {
  if constexpr (ADAM) {
    AdamSlices s = {lin_slice(w), lin_slice(g), lin_slice(m), lin_slice(v), lin_slice(vx)};
    CaF32::step(s, c, live, nans, a_w, a_d);
    lin_unslice(w, s.w);
    lin_unslice(m, s.m);
    lin_unslice(v, s.v);
    lin_unslice(vx, s.x);
  } else {
    CliSlice out;
    if (form)
      CsF32::step<1>(lin_slice(w), lin_slice(g), alpha, live, out, nans, a_w, a_d);
    else
      CsF32::step<0>(lin_slice(w), lin_slice(g), alpha, live, out, nans, a_w, a_d);
    lin_unslice(w, out);
  }
}

// One sample, by its thread: activation, log-softmax, loss, argmax and dz from the partial logits of row `row`
// (summed in wave order) and the bias; dz goes to dzs[row], classes from C on as 0.
__device__ __forceinline__ void lin_sample(const float (*part)[kLinMaxB][16], const float* bias, float (*dzs)[16],
                                           int row, int y, int C, int sigmoid, float inv_b, float& loss,
                                           int& correct) {
  float act[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    float s = part[0][row][c];
#pragma unroll
    for (int p = 1; p < kLinWaves / 2; ++p) s += part[p][row][c];
    const float zc = s + bias[c];
    act[c] = sigmoid ? 1.0f / (1.0f + __builtin_expf(-zc)) : zc;
  }
  float mx = act[0];
  int arg = 0;
#pragma unroll
  for (int c = 1; c < 16; ++c)
    if (c < C && act[c] > mx) {  // strict: a tie keeps the first index
      mx = act[c];
      arg = c;
    }
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    if (c < C) se += __builtin_expf(act[c] - mx);
  const float lse = __builtin_logf(se);
  float ly = 0.f;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    const float ls = (act[c] - mx) - lse;  // log_softmax
    if (c == y) ly = ls;
    const float p = __builtin_expf(ls);
    const float da = p * inv_b - (c == y ? inv_b : 0.f);
    const float dz = sigmoid ? da * act[c] * (1.0f - act[c]) : da;
    dzs[row][c] = c < C ? dz : 0.f;
  }
  loss = -ly;
  correct = arg == y ? 1 : 0;
}
