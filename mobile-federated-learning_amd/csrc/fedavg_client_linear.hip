// fedavg_client_linear.hip -- libfedavg_amd_clientlinear.so (include/
// fedavg_amd_clientlinear.h): the whole local loop of Client.train
// (client.py:52-96) for a model of one affine layer with a cross-entropy
// loss, in one launch of ONE workgroup that stays on its CU for every epoch.
//
// Work split.  512 threads, 8 waves.  D is cut into tiles of
// 16 columns; wave w owns tiles w, w + 8, w + 16, ... (at most 8) for the whole
// loop.  For each of its tiles a lane (i = lane % 16, q = lane / 16) keeps, in
// registers, the four elements (class i, column n0 + 4 q + r), r = 0..3, of
// W, of the gradient (last_grads until the next backward) and of Adam's m, v, vmax.  That is the
// layout v_mfma_f32_16x16x4_f32 leaves its result in, and it is also the
// layout of that instruction's B operand when the four k-indices of one
// instruction are taken to be the columns n0 + 4 q + r of one r: so
//   forward   z[b, c]  += x[b, n0 + 4 q + r] * W[c, n0 + 4 q + r]
//             A = the batch (row b = 16 mt + i, one 16-B LDS read per four
//             instructions), B = W straight from its registers;
//   backward  dW^T[d, c] = sum_b x^T[d, b] * dz[b, c]
//             A = the batch read down a column, B = dz from LDS, the result
//             lands where W lies.
// Neither product ever moves W or its gradient.  Only the [B, 16] partial
// logits cross waves: waves 4..7 write theirs to LDS, waves 0..3 add their
// own on top, and the sample's thread adds the four sums in wave order.
//
// The batch is read from HBM once, into LDS rows of 4 * ceil(D / 4) + 4 floats
// (the + 4 moves consecutive rows to other banks), and BOTH operand layouts
// are read from that one copy: LDS is addressed freely, a transposed second
// copy would not fit next to the first (2 x 128 KiB) and a register copy would
// cost the 64 registers per lane that Adam's state needs.  Above the resident
// size the same two reads go to global memory (L2) instead.
//
// Everything that feeds a reduction runs in a fixed order: a thread's
// elements in tile order, the wave by DPP, the 8 waves in wave order.  The
// arithmetic of the guard, of the steps and of rho / beta is the headers'.
#include "client_adam_rules.hpp"
#include "client_step_rules.hpp"

#include "client_linear_core.hpp"
#include "fedavg_amd_clientlinear.h"

namespace {

thread_local ErrorState g_ln_err;

int ln_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  g_ln_err.vset(code, fmt, ap);
  va_end(ap);
  return code;
}

struct LinArgs {
  float* w;
  float* b;
  const float* x;
  const int64_t* y;
  const double* coef;
  double* rec;
  double lr_ratio;
  float alpha;
  int B, D, C, iters, act, form;
};

template <bool ADAM, bool RES>
__global__ __launch_bounds__(kLinThreads) void client_linear_loop_f32_kernel(const LinArgs a) {
  extern __shared__ __attribute__((aligned(16))) float xs[];
  __shared__ float part[kLinWaves / 2][kLinMaxB][16];  // partial logits
  __shared__ float dzs[kLinMaxB][16];                  // dz; rows from B on stay 0
  __shared__ float lossb[kLinMaxB];
  __shared__ int corr[kLinMaxB];
  __shared__ int ys[kLinMaxB];
  __shared__ float bias[16];
  __shared__ double red[kClientStats][kLinWaves];
  __shared__ float sh_loss;
  __shared__ int sh_correct, sh_flag;
  __shared__ double sh_state[4];  // rho, beta, has rho, has beta: thread 0's

  const int tid = static_cast<int>(threadIdx.x), wave = tid >> 6, lane = tid & 63, i = lane & 15, q = lane >> 4;
  const int B = a.B, D = a.D, C = a.C, D4 = (D + 3) & ~3, S = D4 + 4, MT = (B + 15) >> 4, KS = (B + 3) >> 2;
  const LinBatch<RES> xb = {xs, a.x, B, D, D4, S};

  // ---- the labels, before anything else
  if (tid == 0) {
    sh_flag = 0;
    sh_correct = 0;
    sh_state[0] = sh_state[1] = sh_state[2] = sh_state[3] = 0.0;
  }
  for (int idx = tid; idx < kLinMaxB * 16; idx += kLinThreads) (&dzs[0][0])[idx] = 0.f;
  __syncthreads();
  if (tid < B) {
    const int64_t y = a.y[tid];
    const bool bad = y < 0 || y >= C;
    ys[tid] = bad ? 0 : static_cast<int>(y);
    if (bad) sh_flag = 1;
  }
  __syncthreads();
  if (sh_flag) {
    if (tid == 0) {
      a.rec[0] = -1.0;
#pragma unroll
      for (int j = 1; j < 8; ++j) a.rec[j] = j == 5 ? 1.0 : 0.0;
    }
    return;
  }

  // ---- the batch, once
  if constexpr (RES) {
    const int G = D4 >> 2;
    const bool vec = (D & 3) == 0 && aligned16(a.x);
    for (int idx = tid; idx < B * G; idx += kLinThreads) {
      const int b = idx / G, d = 4 * (idx - b * G);
      const float* src = a.x + static_cast<int64_t>(b) * D;
      f32x4 v;
      if (vec) {
        v = *reinterpret_cast<const f32x4*>(src + d);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float e = src[d + r < D ? d + r : 0];
          v[r] = d + r < D ? e : 0.f;
        }
      }
      *reinterpret_cast<f32x4*>(xs + b * S + d) = v;
    }
  }

  // ---- the parameters and their state, in registers for the whole loop
  float wv[kLinSlots][4], gv[kLinSlots][4];
  float am[ADAM ? kLinSlots : 1][4], av[ADAM ? kLinSlots : 1][4], ax[ADAM ? kLinSlots : 1][4];
  float bw = 0.f, bg = 0.f, bm = 0.f, bv = 0.f, bx = 0.f;
  const int blive = tid < C ? 1 : 0;  // thread c < C owns b[c], as element 0 of a slice
  double acc[kClientStats] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int k = 0; k < kLinSlots; ++k) {
    const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool on = i < C && d0 + r < D;
      const float e = a.w[on ? static_cast<int64_t>(i) * D + d0 + r : 0];
      wv[k][r] = on ? e : 0.f;
      gv[k][r] = 0.f;
      if constexpr (ADAM) am[k][r] = av[k][r] = ax[k][r] = 0.f;
      add_sq(acc[1], static_cast<double>(wv[k][r]));
    }
  }
  if (blive) bw = a.b[tid];
  add_sq(acc[1], static_cast<double>(bw));
  lin_block_sum(acc, red);  // also: the batch and the labels are in LDS
  double sumsq_w = acc[1];  // norm(last_w)^2

  float loss = 0.f, last_loss = 0.f;
  int trip = -1, steps = 0;
  const float inv_b = 1.0f / static_cast<float>(B);

  const int i0 = i, q0 = q;
  for (int ep = 0; ep < a.iters; ++ep) {
    const int i = lin_opaque(i0), q = lin_opaque(q0);
    // ---- forward: this wave's part of z = x W^T
    if (tid < 16) bias[tid] = bw;
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

    // ---- one thread per sample: activation, log-softmax, loss, argmax, dz
    if (tid < B) {
      lin_sample(part, bias, dzs, tid, ys[tid], C, a.act, inv_b, lossb[tid], corr[tid]);
    }
    __syncthreads();

    // ---- the loss, the correct count and db, each by one thread in sample order
    if (tid == 0) {
      double s = 0.0;
      int n = 0;
      for (int b = 0; b < B; ++b) {
        s += static_cast<double>(lossb[b]);
        n += corr[b];
      }
      sh_loss = static_cast<float>(s / static_cast<double>(B));
      sh_correct = n;
    }
    // ---- backward: dW^T = x^T dz for this wave's tiles and db by thread c in sample order, each tile straight
    // into {NaN count, sum g^2, sum (g - last_g)^2}: gv holds last_grads until the new value takes its place (the
    // prologue's last_grads are epoch 0's own)
    int nans = 0;
    acc[0] = acc[1] = acc[2] = 0.0;
    const auto take = [&](float& held, float g) {
      const float d = g - (ep == 0 ? g : held);
      nans += static_cast<int>(g != g);
      add_sq(acc[1], static_cast<double>(g));
      add_sq(acc[2], static_cast<double>(d));
      held = g;
    };
    {
      float s = 0.f;
      if (tid < 16)
        for (int b = 0; b < B; ++b) s += dzs[b][tid];
      take(bg, s);
    }
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int n0 = 16 * (kLinWaves * k + wave);
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (n0 < D) {
        for (int ks = 0; ks < KS; ++ks) g = mfma4(xb.at(4 * ks + q, n0 + i), dzs[4 * ks + q][i], g);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) take(gv[k][r], g[r]);
      __builtin_amdgcn_sched_barrier(0);
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
      const double* t = a.coef + static_cast<int64_t>(kAdamCoefs) * ep;
      c = {static_cast<float>(t[0]), static_cast<float>(t[1]), static_cast<float>(t[2]), static_cast<float>(t[3]),
           static_cast<float>(t[4]), static_cast<float>(t[5]), static_cast<float>(t[6]), a.form, t[0] != 0.0 ? 1 : 0};
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

  // ---- what leaves the CU: the parameters, if a step touched them, and the record
  if (steps > 0) {
#pragma unroll
    for (int k = 0; k < kLinSlots; ++k) {
      const int d0 = 16 * (kLinWaves * k + wave) + 4 * q;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (i < C && d0 + r < D) a.w[static_cast<int64_t>(i) * D + d0 + r] = wv[k][r];
    }
    if (blive) a.b[tid] = bw;
  }
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

bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

template <bool ADAM, bool RES>
int lin_launch(const char* what, const LinArgs& a, int64_t lds, hipStream_t s) {
  const auto kernel = client_linear_loop_f32_kernel<ADAM, RES>;
  if (lds > 32768) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return ln_error(-static_cast<int>(e), "%s: %lld bytes of LDS refused: %s", what, (long long)lds,
                      hipGetErrorString(e));
    }
  }
  hipLaunchKernelGGL(kernel, dim3(1), dim3(kLinThreads), static_cast<size_t>(lds), s, a);
  return launch_status(g_ln_err, what);
}

}  // namespace

extern "C" {

int fedavg_clientlinear_abi_version(void) { return 1; }

const char* fedavg_clientlinear_last_error(void) { return g_ln_err.c_str(); }

void fedavg_client_linear_limits(int64_t* max_b, int64_t* max_d, int64_t* max_c, int64_t* resident_bytes) {
  if (max_b) *max_b = kLinMaxB;
  if (max_d) *max_d = kLinMaxD;
  if (max_c) *max_c = kLinMaxC;
  if (resident_bytes) *resident_bytes = kLinResidentBytes;
}

int fedavg_client_linear_loop_f32(float* w, float* b, const float* x, const int64_t* y, int64_t B, int64_t D,
                                  int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                  double lr_ratio, int form, const double* coef, double* rec, void* stream) {
  const char* what = "fedavg_client_linear_loop_f32";
  if (!w || !b || !x || !y || !rec) return ln_error(FEDAVG_EINVAL, "%s: null w, b, x, y or rec", what);
  if (B < 1 || B > kLinMaxB) return ln_error(FEDAVG_EINVAL, "%s: B = %lld outside [1, %d]", what, (long long)B, kLinMaxB);
  if (D < 1 || D > kLinMaxD) return ln_error(FEDAVG_EINVAL, "%s: D = %lld outside [1, %d]", what, (long long)D, kLinMaxD);
  if (C < 2 || C > kLinMaxC) return ln_error(FEDAVG_EINVAL, "%s: C = %lld outside [2, %d]", what, (long long)C, kLinMaxC);
  if (iters < 0 || iters > INT32_MAX) return ln_error(FEDAVG_EINVAL, "%s: negative iteration count", what);
  if (activation != 0 && activation != 1)
    return ln_error(FEDAVG_EMODE, "%s: activation %d is neither 0 (none) nor 1 (sigmoid)", what, activation);
  if (optimizer != 0 && optimizer != 1)
    return ln_error(FEDAVG_EMODE, "%s: optimizer %d is neither 0 (sgd) nor 1 (adam)", what, optimizer);
  const bool adam = optimizer == 1;
  if (adam ? !adam_form_ok(form) : (form != 0 && form != 1))
    return ln_error(FEDAVG_EMODE, "%s: form %d outside the optimizer's range", what, form);
  if (adam && iters > 0 && !coef) return ln_error(FEDAVG_EINVAL, "%s: null coef", what);
  if (misaligned(w, 4) || misaligned(b, 4) || misaligned(x, 4) || misaligned(y, 8) || misaligned(rec, 8) ||
      (adam && misaligned(coef, 8)))
    return ln_error(FEDAVG_EALIGN, "%s: w, b, x must be 4-B, y, rec and coef 8-B aligned", what);
  if (!is_device_memory(w) || !is_device_memory(b) || !is_device_memory(x) || !is_device_memory(y))
    return ln_error(FEDAVG_EINVAL, "%s: w, b, x and y must be device memory", what);
  if (!is_device_memory(rec) && !is_pinned_host_memory(rec))
    return ln_error(FEDAVG_EINVAL, "%s: rec must be device or pinned host memory", what);
  if (adam && iters > 0) {
    if (!is_pinned_host_memory(coef)) return ln_error(FEDAVG_EINVAL, "%s: coef is not pinned host memory", what);
    for (int64_t t = 0; t < iters; ++t)
      if (!adam_lerp_weight_ok(coef[kAdamCoefs * t + 1]))
        return ln_error(FEDAVG_EMODE, "%s: 1 - beta1 = %g is not below 0.5: the other branch of lerp, not built", what,
                        coef[kAdamCoefs * t + 1]);
  }
  const LinArgs a = {w, b, x, y, coef, rec, lr_ratio, static_cast<float>(-lr),  // ATen: the scalar rounded once to opmath
                     static_cast<int>(B), static_cast<int>(D), static_cast<int>(C), static_cast<int>(iters),
                     activation, form};
  const int64_t need = B * (4 * ((D + 3) / 4) + 4) * 4;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (need <= kLinResidentBytes)
    return adam ? lin_launch<true, true>(what, a, need, s) : lin_launch<false, true>(what, a, need, s);
  return adam ? lin_launch<true, false>(what, a, 0, s) : lin_launch<false, false>(what, a, 0, s);
}

}  // extern "C"
