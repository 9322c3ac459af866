/*
 * fedavg_amd_clientstream.h -- C ABI of libfedavg_amd_clientstream.so: the
 * local loop of fedavg_amd_clientlinear.h (one affine layer, cross-entropy
 * loss, client.py:52-96, ONE launch of one persistent workgroup) for a batch of
 * any realistic length: the batch is walked through the CU in groups of rows
 * that stream through two LDS buffers (csrc/fedavg_client_stream.hip).  fp32
 * model, fp32 batch, int64 labels.
 *
 * The model, the loss, the :71 guard, the SGD and Adam element rules and the
 * rho / beta track are those of fedavg_amd_clientlinear.h, and so is the order
 * of every reduction: the loss is the fp64 sum of the per-sample losses in
 * sample order, db the fp32 sum of dz in sample order, a gradient tile one
 * chain of matrix instructions over 4-sample steps in sample order.  For every
 * shape both entries accept (B <= 64) this entry leaves the bits that
 * fedavg_client_linear_loop_f32 leaves, in w, b and rec.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTSTREAM_H
#define FEDAVG_AMD_CLIENTSTREAM_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientstream_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientstream_last_error(void);

/* The supported range: 1 <= B <= *max_b (16384), 1 <= D <= *max_d (1024),
 * 2 <= C <= *max_c (16).  16384 is a choice, not a bound of the hardware: it
 * keeps B * D within 2^24, so every element index fits 32 bits with room to
 * spare, and it lies far above any client of the reference's datasets.
 * *lds_bytes: the bytes the two row buffers may take together.  A null
 * pointer is skipped.  Host arithmetic. */
void fedavg_client_stream_limits(int64_t* max_b, int64_t* max_d, int64_t* max_c, int64_t* lds_bytes);

/* The rows of a group for batches of D columns: the largest R of 64, 32, 16
 * for which two buffers of R rows of S = 4 * ((D + 3) / 4) + 4 floats,
 * 2 * R * S * 4 bytes, fit *lds_bytes: 64 for D <= 252, 32 for D <= 512, else
 * 16.  0 for a D outside the range.  Host arithmetic. */
int64_t fedavg_client_stream_group_rows(int64_t D);

/*
 * The loop.  w [C, D] and b [C] are updated in place (device fp32, contiguous,
 * 4-B aligned); x [B, D] device fp32; y [B] device int64.  x is read once per
 * epoch; rows that are 16-B aligned (D % 4 == 0 and x 16-B aligned) go from
 * global memory straight into LDS, others are staged through registers.
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
 * index) are that epoch's, from before its step.  All B labels are checked on
 * the device before anything else: for one outside [0, C), label flag = 1, w
 * and b stay untouched, nothing is read or written out of range.  The last
 * group's rows from B on are never read: the caller does not pad.  Adam's m,
 * v, vmax are the workgroup's own (registers, and the values the compiler
 * keeps in its private scratch) and never reach a buffer of the caller.  Two
 * calls on equal inputs leave equal bits.
 *
 * Returns 0, FEDAVG_EINVAL (a null pointer; B, D or C outside the limits; a
 * negative iteration count; memory of the wrong kind), FEDAVG_EALIGN (w, b, x
 * not 4-B or y, rec, coef not 8-B aligned), FEDAVG_EMODE (an unknown
 * activation or optimizer code, a form outside its range, 1 - beta1 not below
 * 0.5).  Nulls, sizes, codes and alignments are validated before any HIP call.
 */
int fedavg_client_linear_stream_f32(float* w, float* b, const float* x, const int64_t* y, int64_t B, int64_t D,
                                    int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                    double lr_ratio, int form, const double* coef, double* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTSTREAM_H */
