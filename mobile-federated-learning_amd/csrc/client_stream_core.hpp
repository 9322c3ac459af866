// client_stream_core.hpp -- the streamed local loop of ONE linear client by ONE workgroup as a device function, with
// the source of the parameters and their destination apart: fedavg_client_cohort.hip runs it once per workgroup,
// from the shared global model into the client's packed row.  The text of the loop is that of the kernel in
// fedavg_client_stream.hip (whose head comment describes it), which keeps its own copy: as a call of this function
// its four instances were allocated differently, and that kernel's code is not to move.  Every
// arithmetic statement and the order of every reduction are the same, so both leave the same bits.  A unit includes
// the rules headers first, as for client_linear_core.hpp.
#pragma once

#include "client_linear_core.hpp"

// One client as its workgroup sees it.  w_in / b_in are read once, before the loop; w_out / b_out are written once,
// after it, and are other memory.
struct StrClient {
  const float* w_in;
  const float* b_in;
  float* w_out;
  float* b_out;
  const float* x;
  const int64_t* y;
  const double* coef;
  double* rec;
  double lr_ratio;
  float alpha;
  int B, D, C, iters, act, form, R;
};

typedef const __attribute__((address_space(1))) void* str_global_ptr;
typedef __attribute__((address_space(3))) void* str_lds_ptr;

// Rows [row0, row0 + rows) of x into `buf`, rows of S floats.  DMA: global memory to LDS, nothing held in registers;
// the caller waits with str_landed().  Else through registers, complete at the next barrier.
template <bool DMA>
__device__ __forceinline__ void str_fetch(const float* x, float* buf, int row0, int rows, int D, int D4, int S) {
  const int tid = static_cast<int>(threadIdx.x);
  if constexpr (DMA) {
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int PR = (D + 255) >> 8;  // pieces of 256 floats per row, the last one masked
    for (int p = wave; p < rows * PR; p += kLinWaves) {
      const int rl = p / PR, d0 = 256 * (p - rl * PR), d = d0 + 4 * lane;
      if (d < D)  // D % 4 == 0: the lane's 16 B lie inside the row
        __builtin_amdgcn_global_load_lds((str_global_ptr)(x + (row0 + rl) * D + d), (str_lds_ptr)(buf + rl * S + d0), 16,
                                         0, 0);
    }
  } else {
    const int G = D4 >> 2;
    for (int idx = tid; idx < rows * G; idx += kLinThreads) {
      const int rl = idx / G, d = 4 * (idx - rl * G);
      const float* src = x + (row0 + rl) * D;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = src[d + r < D ? d + r : 0];
        v[r] = d + r < D ? e : 0.f;
      }
      *reinterpret_cast<f32x4*>(buf + rl * S + d) = v;
    }
  }
}

// this wave's loads to LDS have landed
__device__ __forceinline__ void str_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The loop of client `a` by the calling workgroup of kLinThreads threads.  `xs`: the kernel's dynamic LDS, two
// buffers of R rows of S floats (one suffices for B <= R).  The destination is always written: after a tripped guard
// it holds the parameters as they stood at the trip, after a bad label a copy of the source.
template <bool ADAM, bool DMA>
__device__ __forceinline__ void str_client_loop(const StrClient& a, float* xs) {
  __shared__ float part[kLinWaves / 2][kLinMaxB][16];  // the group's partial logits
  __shared__ float dzs[kLinMaxB][16];                  // the group's dz; rows past its end are 0
  __shared__ float lossb[kLinMaxB];
  __shared__ int corr[kLinMaxB];
  __shared__ float bias[16];
  __shared__ double red[kClientStats][kLinWaves];
  __shared__ float sh_loss;
  __shared__ int sh_correct, sh_flag;
  __shared__ double sh_state[4];  // rho, beta, has rho, has beta: thread 0's

  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int B = a.B, D = a.D, C = a.C, R = a.R, D4 = (D + 3) & ~3, S = D4 + 4, NG = (B + R - 1) / R;

  // ---- the labels, all B of them, before anything else
  if (tid == 0) {
    sh_flag = 0;
    sh_correct = 0;
    sh_state[0] = sh_state[1] = sh_state[2] = sh_state[3] = 0.0;
  }
  __syncthreads();
  for (int b = tid; b < B; b += kLinThreads) {
    const int64_t y = a.y[b];
    if (y < 0 || y >= C) sh_flag = 1;
  }
  __syncthreads();
  if (sh_flag) {
    for (int j = tid; j < C * D; j += kLinThreads) a.w_out[j] = a.w_in[j];  // never left uninitialised
    if (tid < C) a.b_out[tid] = a.b_in[tid];
    if (tid == 0) {
      a.rec[0] = -1.0;
#pragma unroll
      for (int j = 1; j < 8; ++j) a.rec[j] = j == 5 ? 1.0 : 0.0;
    }
    return;
  }

  // ---- group 0 sets out for buffer 0
  str_fetch<DMA>(a.x, xs, 0, B < R ? B : R, D, D4, S);

  // ---- the parameters and their state, in registers for the whole loop
  float wv[kLinSlots][4], gv[kLinSlots][4];
  float am[ADAM ? kLinSlots : 1][4], av[ADAM ? kLinSlots : 1][4], ax[ADAM ? kLinSlots : 1][4];
  f32x4 ga[kLinSlots];  // the epoch's gradient, group by group
  float bw = 0.f, bg = 0.f, bm = 0.f, bv = 0.f, bx = 0.f;
  const int blive = tid < C ? 1 : 0;  // thread c < C owns b[c], as element 0 of a slice
  double acc[kClientStats] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
    ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = i < C && d0 + r < D;
      const float e = a.w_in[on ? i * D + d0 + r : 0];
      wv[k][r] = on ? e : 0.f;
      gv[k][r] = 0.f;
      if constexpr (ADAM) am[k][r] = av[k][r] = ax[k][r] = 0.f;
      add_sq(acc[1], static_cast<double>(wv[k][r]));
    }
  }
  if (blive) bw = a.b_in[tid];
  add_sq(acc[1], static_cast<double>(bw));
  lin_block_sum(acc, red);
  double sumsq_w = acc[1];  // norm(last_w)^2

  float loss = 0.f, last_loss = 0.f;
  int trip = -1, steps = 0;
  int t = 0;  // groups walked: with more than one group, group number t of the walk lies in buffer t & 1
  const float inv_b = 1.0f / static_cast<float>(B);

  const int i0 = i, q0 = q;
  for (int ep = 0; ep < a.iters; ++ep) {
    const int i = lin_opaque(i0), q = lin_opaque(q0);
    if (tid < 16) bias[tid] = bw;
    double loss_sum = 0.0;  // thread 0's, in sample order across the groups
    int correct = 0;
    float db = 0.f;  // thread c's sum of dz[., c], in sample order across the groups

    for (int c = 0; c < NG; ++c, ++t) {
      const int row0 = c * R, rows = B - row0 < R ? B - row0 : R;
      const int MT = (rows + 15) >> 4, KS = (rows + 3) >> 2;
      float* cur = xs + (NG > 1 && (t & 1) ? R * S : 0);
      // ---- S0: this group's rows are in `cur`, and no wave still reads the other buffer
      if constexpr (DMA) str_landed();
      __syncthreads();
      if (NG > 1 && !(c + 1 == NG && ep + 1 == a.iters)) {
        const int n0 = c + 1 == NG ? 0 : row0 + R;
        str_fetch<DMA>(a.x, xs + (t & 1 ? 0 : R * S), n0, B - n0 < R ? B - n0 : R, D, D4, S);
      }
      const LinBatch<true> xb = {cur, a.x, rows, D, D4, S};

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
        const int64_t y = a.y[row0 + tid];  // checked above; compared, never an index
        lin_sample(part, bias, dzs, tid, static_cast<int>(y), C, a.act, inv_b, lossb[tid], corr[tid]);
      } else if (tid < kLinMaxB) {
#pragma unroll
        for (int cc = 0; cc < 16; ++cc) dzs[tid][cc] = 0.f;
      }
      __syncthreads();

      // ---- the loss and the correct count by thread 0, db by thread c, the tiles' x^T dz: all in sample order
      if (tid == 0) {
        for (int b = 0; b < rows; ++b) {
          loss_sum += static_cast<double>(lossb[b]);
          correct += corr[b];
        }
      }
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

    // ---- the epoch's gradient is complete: {NaN count, sum g^2, sum (g - last_g)^2}; gv holds last_grads until
    // the new value takes its place (the prologue's last_grads are epoch 0's own)
    if (tid == 0) {
      sh_loss = static_cast<float>(loss_sum / static_cast<double>(B));
      sh_correct = correct;
    }
    int nans = 0;
    acc[0] = acc[1] = acc[2] = 0.0;
    const auto take = [&](float& held, float g) {
      const float d = g - (ep == 0 ? g : held);
      nans += static_cast<int>(g != g);
      add_sq(acc[1], static_cast<double>(g));
      add_sq(acc[2], static_cast<double>(d));
      held = g;
    };
    take(bg, db);
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
#pragma unroll
      for (int r = 0; r < 4; ++r) take(gv[k][r], ga[k][r]);
      ga[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    acc[0] = static_cast<double>(nans);
    lin_block_sum(acc, red);
    loss = sh_loss;
    if (ep == 0) last_loss = loss;

    // ---- the :71 guard, the same decision in every thread
    const double n_g = guard_norm<CliOpF32>(acc[1]), n_w = guard_norm<CliOpF32>(sumsq_w);
    if (acc[0] > 0.0 || loss != loss || n_g > guard_bound<CliOpF32>(n_w, a.lr_ratio)) {
      trip = ep;
      break;
    }

    // ---- the step
    AdamCoef<float> c = {};
    if constexpr (ADAM) {
      const double* tc = a.coef + static_cast<int64_t>(kAdamCoefs) * ep;
      c = {static_cast<float>(tc[0]), static_cast<float>(tc[1]), static_cast<float>(tc[2]), static_cast<float>(tc[3]),
           static_cast<float>(tc[4]), static_cast<float>(tc[5]), static_cast<float>(tc[6]), a.form, tc[0] != 0.0 ? 1 : 0};
    }
    double wst[4] = {0.0, 0.0, 0.0, 0.0};
    int wn = 0;
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int left = D - (16 * (kLinWaves * k + wave) + 4 * q);
      const int live = i < C ? (left < 0 ? 0 : left > 4 ? 4 : left) : 0;
      lin_step<ADAM>(wv[k], gv[k], am[ADAM ? k : 0], av[ADAM ? k : 0], ax[ADAM ? k : 0], a.alpha, a.form, c, live, wn,
                     wst[1], wst[2]);
      __builtin_amdgcn_sched_barrier(0);
    }
    {
      float w4[4] = {bw, 0.f, 0.f, 0.f}, g4[4] = {bg, 0.f, 0.f, 0.f}, m4[4] = {bm, 0.f, 0.f, 0.f},
            v4[4] = {bv, 0.f, 0.f, 0.f}, x4[4] = {bx, 0.f, 0.f, 0.f};
      lin_step<ADAM>(w4, g4, m4, v4, x4, a.alpha, a.form, c, blive, wn, wst[1], wst[2]);
      bw = w4[0], bm = m4[0], bv = v4[0], bx = x4[0];
    }
    double wacc[kClientStats] = {static_cast<double>(wn), wst[1], wst[2]};
    lin_block_sum(wacc, red);
    wst[0] = wacc[0];
    wst[1] = wacc[1];
    wst[2] = wacc[2];
    sumsq_w = wacc[1];

    // ---- rho / beta (:78-84)
    if (tid == 0)
      cli_track<CliOpF32>(sh_state, wst, acc,
                          __builtin_fabs(static_cast<double>(loss) - static_cast<double>(last_loss)));
    last_loss = loss;
    ++steps;
  }
  if constexpr (DMA) str_landed();  // a tripped guard leaves the next epoch's first group on its way

  // ---- what leaves the CU: the parameters, whether or not a step touched them, and the record
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (i < C && d0 + r < D) a.w_out[i * D + d0 + r] = wv[k][r];
  }
  if (blive) a.b_out[tid] = bw;
  if (tid == 0) {
    a.rec[0] = static_cast<double>(trip);
    a.rec[1] = static_cast<double>(loss);
    a.rec[2] = sh_state[1];
    a.rec[3] = sh_state[0];
    a.rec[4] = static_cast<double>(sh_correct);
    a.rec[5] = 0.0;
    a.rec[6] = static_cast<double>(steps);
    a.rec[7] = 0.0;
  }
}
