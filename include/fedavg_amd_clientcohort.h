/*
 * fedavg_amd_clientcohort.h -- C ABI of libfedavg_amd_clientcohort.so: the
 * local loops of all the linear softmax clients of a round
 * (fedavg_trainer.py:172-199: each trained from the same global model) in ONE
 * launch, one persistent workgroup per client, each client's trained model
 * written into its row of the packed client-major [K, ld] buffer that
 * fedavg_reduce_f32 / fedavg_reduce_sqdist_f32 read
 * (csrc/fedavg_client_cohort.hip).  fp32 model, fp32 batches, int64 labels.
 *
 * A workgroup is the streamed loop of fedavg_amd_clientstream.h: the model, the
 * loss, the :71 guard, the SGD and Adam element rules, the rho / beta track and
 * the order of every reduction are that entry's.  For every client k, row k
 * and record k hold the bits fedavg_client_linear_stream_f32 leaves when run
 * alone on that client from `model` (and so, for B_k <= 64, those of
 * fedavg_client_linear_loop_f32).
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTCOHORT_H
#define FEDAVG_AMD_CLIENTCOHORT_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientcohort_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientcohort_last_error(void);

/* The supported range: 1 <= K <= *max_k (4096: a choice that keeps the table
 * and the records small), and per client the range of
 * fedavg_client_stream_limits: 1 <= B <= *max_b (16384), 1 <= D <= *max_d
 * (1024), 2 <= C <= *max_c (16).  A null pointer is skipped.  Host
 * arithmetic. */
void fedavg_client_cohort_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c);

/*
 * The cohort.  With P = C * D + C:
 *   model   : the global model, P fp32 in device memory in state_dict order
 *             (weight [C, D], then bias [C]), 4-B aligned; read, never written
 *   rows    : device fp32 [K, ld], ld >= P, 4-B aligned.  Client k's trained
 *             weight and bias go to rows + k * ld in the order of `model`;
 *             columns [P, ld) are not written
 *   clients : K entries of 32 bytes
 *                 { const float* x; const int64_t* y; int64_t B; int64_t row; }
 *             in PINNED HOST memory, 8-B aligned: the host validates the table
 *             and the kernel reads it where it lies.  PRECONDITION: `clients`
 *             is an address the calling thread can read, K * 32 bytes of it.
 *             The table's contents are validated before any HIP call, hence
 *             before the library can ask what kind of memory it is: a device
 *             pointer, or any address that is not mapped on the host, is not
 *             refused but faults the caller.  Host memory that is readable
 *             but not pinned is refused.  Workgroup g trains entry g and writes row and
 *             record `row`; the `row` values are a permutation of 0 .. K - 1,
 *             so the caller may order the entries (longest batch first, since
 *             the hardware starts workgroups in order) without moving rows.
 *             x [B, D] fp32 and y [B] int64 are device memory, 1 <= B <= max_b
 *   rec     : [K, 8] doubles, device or pinned host memory, 8-B aligned;
 *             record `row` has the fields of fedavg_client_linear_stream_f32:
 *             {trip epoch or -1, loss, beta, rho, correct count, label flag,
 *              steps taken, 0}
 *   iters, activation, optimizer, lr, lr_ratio, form, coef: as in
 *             fedavg_client_linear_stream_f32, shared by the cohort
 * Every row is written, whatever became of its client: after a tripped guard
 * it holds the parameters as they stood at the trip, and for a client with a
 * label outside [0, C) (label flag = 1) a copy of `model`.  One client's bad
 * label or NaN touches no other client's row or record.  Rows go from global
 * memory straight into LDS when D % 4 == 0 and every x is 16-B aligned,
 * otherwise every client's rows are staged through registers; the bits do not
 * depend on which.  Two calls on equal inputs leave equal bits.
 *
 * Returns 0, FEDAVG_EINVAL (a null pointer, also inside an entry; K, D, C or an
 * entry's B outside the limits; ld < P; a negative iteration count; a `row`
 * outside [0, K) or used twice; memory of the wrong kind: a table that is not
 * pinned, an x or y that is not device memory), FEDAVG_EALIGN (model, rows or an
 * x not 4-B, clients, rec, coef or a y not 8-B aligned), FEDAVG_EMODE (an unknown
 * activation or optimizer code, a form outside its range, 1 - beta1 not below
 * 0.5).  Nulls, sizes, codes, alignments and the table's contents are validated
 * before any HIP call, and everything before the launch.
 */
int fedavg_client_cohort_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K, int64_t D,
                             int64_t C, int64_t iters, int activation, int optimizer, double lr, double lr_ratio,
                             int form, const double* coef, double* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTCOHORT_H */
