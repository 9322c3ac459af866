/*
 * fedavg_amd_clienteval.h -- C ABI of libfedavg_amd_clienteval.so: the
 * evaluation of one linear softmax model on every client's whole dataset
 * (fedavg_trainer.py:461-529, one Client.local_test of client.py:99-120 per
 * client and per set) in ONE call: a setup launch, one persistent forward
 * kernel over all the clients' rows, a finish launch
 * (csrc/fedavg_client_eval.hip).  fp32 model, fp32 batches, int64 labels.
 *
 * Forward only.  The model is that of fedavg_amd_clientcohort.h (one affine
 * layer, an optional sigmoid after it, cross-entropy on the result), and the
 * fp32 arithmetic of one sample is the training kernels': with a = the
 * activations and mx their maximum, the loss is -((a[y] - mx) - log(sum exp(a -
 * mx))).  One thing differs on purpose: the ARGMAX follows torch.max, which is
 * what local_test calls -- the lowest index among equal maxima, and a NaN
 * beats every number, the first NaN winning -- while the training kernels'
 * correct count uses a strict `>` from index 0, under which a NaN never wins.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTEVAL_H
#define FEDAVG_AMD_CLIENTEVAL_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clienteval_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clienteval_last_error(void);

/* The supported range, that of fedavg_client_cohort_limits: 1 <= K <= *max_k
 * (4096), and per client 1 <= B <= *max_b (16384), 1 <= D <= *max_d (1024),
 * 2 <= C <= *max_c (16).  A null pointer is skipped.  Host arithmetic. */
void fedavg_client_eval_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c);

/* Bytes of `workspace` that fedavg_client_eval_f32 needs for this table: with
 * chunks = sum over the entries of ceil(B / 256) (a chunk is a run of at most
 * 256 rows of one client, the kernel's unit of work),
 *     roundup(4 * (K + 1), 32) + 32 * K + 32 * chunks
 * (the chunk prefix table, a device copy of the table, one 32-B partial per
 * chunk).  `clients` is read on the host as the entry reads it; D is accepted
 * for the ABI's sake and does not change the result today.  Returns
 * FEDAVG_EINVAL (negative) for a null table or a K, D or B outside the limits.
 * Host arithmetic. */
int64_t fedavg_client_eval_workspace_bytes(const void* clients, int64_t K, int64_t D);

/*
 * The evaluation.  With P = C * D + C:
 *   model    : P fp32 in device memory in state_dict order (weight [C, D],
 *              then bias [C]), 4-B aligned; read, never written
 *   clients  : K entries of 32 bytes
 *                  { const float* x; const int64_t* y; int64_t B; int64_t slot; }
 *              in PINNED HOST memory, 8-B aligned, validated on the host exactly
 *              as fedavg_client_cohort_f32 validates its table, under the same
 *              PRECONDITION: `clients` is an address the calling thread can
 *              read, K * 32 bytes of it.  x [B, D] fp32 and y [B] int64 are
 *              device memory.  The `slot` values are a permutation of
 *              0 .. K - 1: entry g's result goes to record `slot`, so the caller
 *              may order the entries (longest first) without moving records.
 *              No record depends on the order of the entries.
 *   activation : 0 (none) or 1 (sigmoid after the affine layer)
 *   rec      : [K, 4] doubles, device or pinned host memory, 8-B aligned;
 *              record `slot` = {sum over the client's samples of the per-sample
 *              cross-entropy (what local_test reports: loss.item() * B),
 *              correct count, label flag, B}
 *   workspace, workspace_bytes : device memory, 16-B aligned, at least
 *              fedavg_client_eval_workspace_bytes(clients, K, D) bytes; need
 *              not be cleared; every byte the call reads it has written
 * Tails in B, D and C are masked; nothing is padded by the caller.  A label
 * outside [0, C) sets its client's label flag and that sample adds nothing to
 * the loss or the count; a NaN in an x makes that client's loss NaN; neither
 * touches another client's record.  Rows are loaded 16 B at a time when
 * D % 4 == 0 and every x is 16-B aligned, else the whole launch loads single
 * floats; the bits do not depend on which, nor on the number of workgroups.
 * Loss sums are fp64 and counts integers, added in one fixed order with no
 * atomics: two calls on equal inputs leave equal bits.
 *
 * Returns 0, FEDAVG_EINVAL (a null pointer, also inside an entry; K, D, C or an
 * entry's B outside the limits; a `slot` outside [0, K) or used twice; a
 * workspace below the size above; memory of the wrong kind: a table that is
 * not pinned, a model, workspace, x or y that is not device memory),
 * FEDAVG_EALIGN (model or an x not 4-B, clients, rec or a y not 8-B, workspace not
 * 16-B aligned), FEDAVG_EMODE (an unknown activation code).  Nulls, sizes, codes,
 * alignments and the table's contents are validated before any HIP call, and
 * everything before the first launch.
 */
int fedavg_client_eval_f32(const float* model, const void* clients, int64_t K, int64_t D, int64_t C, int activation,
                           double* rec, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTEVAL_H */
