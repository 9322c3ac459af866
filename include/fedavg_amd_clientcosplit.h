/*
 * fedavg_amd_clientcosplit.h -- C ABI of libfedavg_amd_clientcosplit.so: the
 * local loops of ALL the linear clients of a round (fedavg_trainer.py:172-199)
 * with EACH CLIENT'S BATCH SPLIT ACROSS WORKGROUPS
 * (csrc/fedavg_client_cosplit.hip).  The contract is that of
 * fedavg_client_cohort_f32 (fedavg_amd_clientcohort.h), plus a workspace and
 * the number of slices a workgroup walks: every client trained from the same
 * model for `iters` local iterations under the :71 guard, client `row` into
 * row `row` of the packed buffer the reduce reads, one record of eight fields
 * per client.  fp32 model, fp32 batches, int64 labels.
 *
 * Where the cohort is one persistent workgroup per client, a local iteration
 * here is two launches over ALL clients, enqueued back to back on `stream`
 * with no host sync between iterations:
 *   setup    : once.  Workgroup g checks every label of entry g, copies
 *              `model` into the entry's row, zeroes the client's state block
 *              and writes its record; one more workgroup lays out the group
 *              table.  With R = the slice height (below), G_k = ceil(B_k / R)
 *              and q = slices_per_group, client k has n_k = ceil(G_k / q)
 *              workgroups and workgroup j of it owns slices
 *              [j q, min((j + 1) q, G_k)).
 *   gradient : sum_k n_k workgroups.  A workgroup reads its (entry, first
 *              slice) from the group table, loads W and b from its client's
 *              row, brings its slices into LDS one after another (ONE buffer:
 *              a slice of R rows fills the LDS budget), forms their logits
 *              and dz^T x with the 16x16x4 fp32 matrix instruction, dW
 *              accumulating in registers in slice order, and writes one slot
 *              of the plane: dW, db, its fp64 loss sum in sample order and
 *              its correct count
 *   step     : one workgroup per client.  It sums its client's n_k slots in
 *              slot order in fp32, forms the guard's sums, decides the guard,
 *              applies the SGD or Adam element rule to the row (Adam's m, v,
 *              vmax in the workspace), tracks rho / beta, keeps the gradient
 *              as last_grads and, after the last iteration or at a trip,
 *              writes the record
 * A client with a bad label or a tripped guard is inert for the rest of the
 * call: its workgroups return at once.  No workgroup waits for another, there
 * is no atomic and every sum has a fixed order.
 *
 * The slice height R is fedavg_client_split_slice_rows(D)'s
 * (fedavg_amd_clientsplit.h): the most rows of 4 * ceil(D / 4) + 4 floats, in
 * multiples of 16 and at most 256, that fit the LDS budget
 * fedavg_client_stream_limits reports; 32 at D = 784.
 *
 * Bit contract:
 *   - row k and record k are a function of client k's inputs, `model`, the
 *     hyper-parameters and slices_per_group alone: they do not depend on the
 *     other clients, on the table's order or on K;
 *   - two calls on equal inputs leave equal bits;
 *   - the results are NOT the one-workgroup cohort's bits: a client's
 *     gradient is summed slot by slot here, and in one run of sample order
 *     there;
 *   - nothing past workspace_bytes is touched and columns [P, ld) of a row
 *     are not written.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTCOSPLIT_H
#define FEDAVG_AMD_CLIENTCOSPLIT_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientcosplit_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientcosplit_last_error(void);

/* The bytes of workspace a call needs for clients of B[0 .. K) rows.  With
 * N = sum_k n_k (above), P = C * D + C and a = 1 for Adam (optimizer 1), 0 for
 * SGD (optimizer 0):
 *     104 K + 24 N + 4 P (N + K (1 + 3 a))
 * per client its table entry (32), its state block (64) and its span of slots
 * (8), per workgroup its group entry (8), its loss sum and correct count (16)
 * and its slot of the plane (4 P), per client last_grads (4 P) and Adam's
 * m, v, vmax (12 P).  0 for a null B, K outside [1, 4096], a B[k] outside
 * [1, 16384], D outside [1, 1024], C outside [2, 16], slices_per_group < 1 or
 * an optimizer that is neither.  Host arithmetic. */
int64_t fedavg_client_cosplit_workspace_bytes(const int64_t* B, int64_t K, int64_t D, int64_t C,
                                              int64_t slices_per_group, int optimizer);

/*
 * The cohort, batch-split.  model, rows, ld, clients (the 32-B pinned entries
 * {x, y, B, row}, `row` a permutation of 0 .. K - 1), K, D, C, iters,
 * activation, optimizer, lr, lr_ratio, form, coef and rec ([K, 8]: trip epoch
 * or -1, loss, beta, rho, correct count, label flag, steps taken, 0) are
 * those of fedavg_client_cohort_f32, with its ranges (K <= 4096, B <= 16384,
 * D <= 1024, 2 <= C <= 16).  The table and `coef` are read on the calling
 * thread while the launches are enqueued and the table by the setup launch on
 * the device.  While the call's launches run, a row holds its client's
 * parameters as of the last finished step.
 *   slices_per_group: q >= 1, the slices one workgroup of the gradient launch
 *                     walks
 *   workspace       : device memory, 8-B aligned, of `workspace_bytes` bytes,
 *                     at least fedavg_client_cosplit_workspace_bytes(the
 *                     table's B, K, D, C, slices_per_group, optimizer); its
 *                     contents on entry do not matter
 * The call enqueues 1 + 2 * iters launches.  A client with a label outside
 * [0, C) gets label flag 1 and a copy of `model` in its row and touches no
 * other client; a client whose guard trips keeps in its row the parameters at
 * the trip.  Rows go from global memory straight into LDS when D % 4 == 0 and
 * every x is 16-B aligned, otherwise every slice is staged through registers;
 * the bits do not depend on which.  Loss and correct count are the last
 * epoch's, from before its step.
 *
 * Returns what fedavg_client_cohort_f32 returns for the same arguments, in the
 * same order of checks; FEDAVG_EINVAL for slices_per_group < 1, for a null
 * workspace, one smaller than fedavg_client_cosplit_workspace_bytes or not
 * device memory; FEDAVG_EALIGN for one not 8-B aligned.  Nulls, sizes, codes,
 * alignments, the table's contents and the workspace's size are validated
 * before any HIP call, and everything before the first launch.
 */
int fedavg_client_cohort_split_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K,
                                   int64_t D, int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                   double lr_ratio, int form, const double* coef, double* rec,
                                   int64_t slices_per_group, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTCOSPLIT_H */
