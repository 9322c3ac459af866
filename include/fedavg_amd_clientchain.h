/*
 * fedavg_amd_clientchain.h -- C ABI of libfedavg_amd_clientchain.so: the chain
 * of optimizer steps of FedAvgTrainer.central_train (fedavg_trainer.py:361-371)
 * for a linear softmax model in ONE launch of one persistent workgroup
 * (csrc/fedavg_client_chain.hip): one model, one step on the whole batch of
 * each entry of a client table, in table order, the table walked `rounds`
 * times, the optimizer state carried from step to step and from call to call.
 * fp32 model, fp32 batches, int64 labels.
 *
 * The model, the loss and the SGD and Adam element rules are those of
 * fedavg_amd_clientstream.h, and so is the order of every reduction within a
 * step: one step from parameters w on batch k leaves the bits that
 * fedavg_client_linear_stream_f32 with iters = 1 leaves from w on that batch
 * when its guard does not trip.  There is no :71 guard here, no rho / beta and
 * no accuracy: central_train has none.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTCHAIN_H
#define FEDAVG_AMD_CLIENTCHAIN_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientchain_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientchain_last_error(void);

/* The supported range, that of fedavg_client_cohort_limits: 1 <= K <= *max_k
 * (4096), and per entry 1 <= B <= *max_b (16384), 1 <= D <= *max_d (1024),
 * 2 <= C <= *max_c (16).  A null pointer is skipped.  Host arithmetic. */
void fedavg_client_chain_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c);

/*
 * The chain.  With P = C * D + C:
 *   model   : P fp32 in device memory in state_dict order (weight [C, D], then
 *             bias [C]), 4-B aligned; updated in place, written once, after the
 *             call's last step
 *   state   : Adam only (null for SGD): 3 P fp32 in device memory, 4-B aligned,
 *             the planes m, v, vmax in the order of `model`; read at entry
 *             unless step0 == 0 (then the planes count as zero, as in the first
 *             step of fedavg_client_adam_step_*) and written at exit
 *   clients : K entries of 32 bytes
 *                 { const float* x; const int64_t* y; int64_t B; int64_t unused; }
 *             in PINNED HOST memory, 8-B aligned, under the precondition of
 *             fedavg_amd_clientcohort.h: an address the calling thread can
 *             read, K * 32 bytes of it; the table's contents are validated
 *             before any HIP call.  x [B, D] fp32 and y [B] int64 are device
 *             memory.  The table is WALKED IN ITS ORDER: the order is the
 *             algorithm, nothing is sorted
 *   rounds  : >= 1, rounds * K <= 2^31 - 1: the table is walked `rounds`
 *             times, rounds * K steps
 *   step0   : >= 0, the steps earlier calls took: Adam's step number of the
 *             call's i-th step (from 0) is step0 + i + 1
 *   coef    : Adam only: rounds * K rows of the 7 coefficients of
 *             fedavg_client_adam_step_*, row i for the call's step i; device or
 *             pinned host memory, 8-B aligned.  Pinned rows are validated on
 *             the host (1 - beta1 below 0.5); device rows are not read there
 *   activation, optimizer, lr, form: as in fedavg_client_linear_stream_f32
 *   losses  : `rounds` doubles, device or pinned host memory, 8-B aligned:
 *             entry r is the loss of the last table entry's batch in round r,
 *             from before its step (what :372 logs)
 *   rec     : 8 doubles, device or pinned host memory, 8-B aligned:
 *             {label flag, first table entry with a bad label or -1,
 *              steps taken, last loss, 0, 0, 0, 0}
 * All labels of all entries are checked on the device before the first step:
 * if one lies outside [0, C), label flag = 1, the lowest such entry is
 * reported, model and state stay untouched and nothing is read out of range.
 * A NaN is not guarded against (the reference has no guard here): it goes into
 * the model.  Rows go from global memory straight into LDS when D % 4 == 0 and
 * every x is 16-B aligned, otherwise every batch is staged through registers;
 * the bits do not depend on which.  Two calls on equal inputs leave equal
 * bits.
 *
 * Returns 0, FEDAVG_EINVAL (a null pointer, also inside an entry; K, D, C, an
 * entry's B, rounds or step0 outside their ranges; Adam without state or coef;
 * memory of the wrong kind), FEDAVG_EALIGN (model, state or an x not 4-B,
 * clients, losses, rec, coef or a y not 8-B aligned), FEDAVG_EMODE (an unknown
 * activation or optimizer code, a form outside its range, 1 - beta1 not below
 * 0.5 in a pinned coef).  Nulls, sizes, codes, alignments and the table's
 * contents are validated before any HIP call, and everything before the
 * launch.
 */
int fedavg_client_chain_f32(float* model, float* state, const void* clients, int64_t K, int64_t D, int64_t C,
                            int64_t rounds, int64_t step0, int activation, int optimizer, double lr, int form,
                            const double* coef, double* losses, double* rec, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTCHAIN_H */
