/*
 * fedavg_amd_clientlinear.h -- C ABI of libfedavg_amd_clientlinear.so: the
 * whole local loop of Client.train (client.py:52-96) for a client whose model
 * is one affine layer with a cross-entropy loss, in ONE launch of one
 * persistent workgroup (csrc/fedavg_client_linear.hip).  fp32 model, fp32
 * batch, int64 labels.
 *
 *   z = x W^T + b;  a = z (activation 0) or sigmoid(z) (activation 1)
 *   loss = mean_i(logsumexp(a_i) - a_i[y_i])
 *   da = (softmax(a) - onehot(y)) / B;  dz = da (0) or da * a * (1 - a) (1)
 *   dW = dz^T x;  db = sum_i dz_i
 *
 * Per epoch, as client.py:58-86: the :71 guard (a NaN gradient, a NaN loss,
 * norm(g) > lr_ratio * norm(last_w)), the step, then rho / beta; the
 * prologue's last_loss / last_grads are the first epoch's own values.  The
 * guard, the SGD and Adam element rules and the rho / beta track are the ones
 * of fedavg_amd_clientloop.h / clientstep.h / clientadam.h: given the same
 * gradients the step leaves the same bits.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTLINEAR_H
#define FEDAVG_AMD_CLIENTLINEAR_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientlinear_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientlinear_last_error(void);

/* The supported range: 1 <= B <= *max_b, 1 <= D <= *max_d, 2 <= C <= *max_c.
 * The batch stays in LDS for the whole loop when
 * B * (4 * ((D + 3) / 4) + 4) * 4 <= *resident_bytes, which holds for every
 * B * D <= 32 * 1024 inside the range; above it the batch is re-read from L2
 * every epoch.  A null pointer is skipped.  Host arithmetic. */
void fedavg_client_linear_limits(int64_t* max_b, int64_t* max_d, int64_t* max_c, int64_t* resident_bytes);

/*
 * The loop.  w [C, D] and b [C] are updated in place (device fp32, contiguous,
 * 4-B aligned); x [B, D] device fp32; y [B] device int64.
 *   iters      : local_iteration >= 0 (0: only the record is written)
 *   activation : 0 none, 1 sigmoid
 *   optimizer  : 0 plain SGD (lr), 1 Adam with amsgrad (coef)
 *   lr_ratio   : the caller's lr * THRESHOLD_GRADS_RATIO, formed in fp64
 *   form       : SGD: 0 / 1 as fedavg_client_sgd_step_*; Adam: the mask 0..15
 *                of fedavg_client_adam_step_*
 *   coef       : Adam only: iters rows of the 7 coefficients of
 *                fedavg_client_adam_step_* (row t for step t + 1), in PINNED
 *                HOST memory: the host validates it and the kernel reads it
 *                where it lies; the device evaluates no pow
 *   rec        : 8 doubles, device or pinned host memory, 8-B aligned:
 *                {trip epoch or -1, loss, beta, rho, correct count,
 *                 label flag, steps taken, 0}
 * A tripped guard ends the loop before that epoch's step.  After the last
 * epoch loss and the correct count (argmax(a_i) == y_i, a tie takes the first
 * index) are that epoch's, from before its step.  A label outside [0, C) is
 * found on the device before anything else: label flag = 1, w and b stay
 * untouched, nothing is read or written out of range.  Adam's m, v, vmax are
 * the workgroup's own (registers, and the few values the compiler keeps in its
 * private scratch) and never reach a buffer of the caller.  Two calls on equal
 * inputs leave equal bits.
 *
 * Returns 0, FEDAVG_EINVAL (a null pointer; B, D or C outside the limits; a
 * negative iteration count; memory of the wrong kind), FEDAVG_EALIGN (w, b, x
 * not 4-B or y, rec, coef not 8-B aligned), FEDAVG_EMODE (an unknown
 * activation or optimizer code, a form outside its range, 1 - beta1 not below
 * 0.5).  Nulls, sizes, codes and alignments are validated before any HIP call.
 */
int fedavg_client_linear_loop_f32(float* w, float* b, const float* x, const int64_t* y, int64_t B, int64_t D,
                                  int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                  double lr_ratio, int form, const double* coef, double* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTLINEAR_H */
