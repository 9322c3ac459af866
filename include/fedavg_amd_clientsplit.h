/*
 * fedavg_amd_clientsplit.h -- C ABI of libfedavg_amd_clientsplit.so: the chain
 * of optimizer steps of FedAvgTrainer.central_train (fedavg_trainer.py:361-371)
 * for a linear softmax model with EACH STEP'S BATCH SPLIT ACROSS WORKGROUPS
 * (csrc/fedavg_client_split.hip).  The contract is that of
 * fedavg_client_chain_f32 (fedavg_amd_clientchain.h), plus a workspace: one
 * model, one step on the whole batch of each entry of a client table, in table
 * order, the table walked `rounds` times, the optimizer state carried from step
 * to step and from call to call.  fp32 model, fp32 batches, int64 labels.
 *
 * Where the chain is one persistent workgroup, a step here is two launches,
 * enqueued back to back on `stream` with no host sync between steps:
 *   gradient : ceil(B / R) workgroups, R = fedavg_client_split_slice_rows(D).
 *              Workgroup g brings rows [g R, min(B, (g + 1) R)) of x into LDS
 *              once, forms their logits and the slice's dz^T x with the
 *              16x16x4 fp32 matrix instruction and writes its partial dW, its
 *              partial db and its fp64 loss sum to slot g of the workspace
 *   step     : each thread sums the slots of its four parameters in slot order
 *              0 .. G - 1 in fp32 and applies the SGD or Adam element rule to
 *              W and b (and m, v, vmax in `state`) in global memory; one thread
 *              adds the fp64 loss sums in slot order and writes losses / rec
 * One launch before the first step checks every label of every entry and
 * leaves the verdict in a word of the workspace, which every later launch of
 * the call reads first.  No workgroup waits for another, there is no atomic
 * and every sum has a fixed order: the result is a function of the inputs
 * alone, and two calls on equal inputs leave equal bits.
 *
 * The model, the loss and the element rules are those of the chain.  The
 * result does NOT have the chain's bits: a step's gradient is summed slice by
 * slice here and in one run of sample order there.  Within a slice the order
 * is the chain's.
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTSPLIT_H
#define FEDAVG_AMD_CLIENTSPLIT_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientsplit_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientsplit_last_error(void);

/* The rows R of one slice at D columns: a multiple of 16 and a function of D
 * alone: the most rows (at most 256) of 4 * ceil(D / 4) + 4 floats that fit the
 * LDS budget fedavg_client_stream_limits reports.  0 for D outside [1, 1024].
 * Host arithmetic. */
int64_t fedavg_client_split_slice_rows(int64_t D);

/* The bytes of workspace a call needs whose table's largest batch has max_B
 * rows: with G = ceil(max_B / R) and P = C * D + C, 256 + 8 G + 4 G P.  0 for
 * max_B outside [1, 16384], D outside [1, 1024] or C outside [2, 16].  Host
 * arithmetic. */
int64_t fedavg_client_split_workspace_bytes(int64_t max_B, int64_t D, int64_t C);

/*
 * The chain, batch-split.  model, state, clients, K, D, C, rounds, step0,
 * activation, optimizer, lr, form, coef, losses and rec are those of
 * fedavg_client_chain_f32, with its ranges (K <= 4096, B <= 16384, D <= 1024,
 * 2 <= C <= 16), except that `model` and `state` are read and written by every
 * step: while the call's launches run they hold the parameters as of the last
 * finished step.  The table is WALKED IN ITS ORDER and is read on the calling
 * thread while the launches are enqueued and by the label check on the device.
 *   workspace       : device memory, 8-B aligned, of `workspace_bytes` bytes,
 *                     at least fedavg_client_split_workspace_bytes(the table's
 *                     largest B, D, C); its contents on entry do not matter
 *                     and nothing past workspace_bytes is touched
 * The call enqueues 1 + 2 * rounds * K launches.  All labels of all entries are
 * checked on the device before the first step: if one lies outside [0, C),
 * rec = {1, the lowest such entry, 0, ...}, every later launch of the call
 * does nothing, model and state stay untouched and nothing is read out of
 * range.  Rows go from global memory straight into LDS when D % 4 == 0 and
 * every x is 16-B aligned, otherwise every slice is staged through registers;
 * the bits do not depend on which.  The result does not depend on how a run of
 * rounds is cut into calls (step0, state and coef carried), to the bit.
 *
 * Returns what fedavg_client_chain_f32 returns for the same arguments, in the
 * same order of checks, and FEDAVG_EINVAL for a null workspace, one smaller
 * than fedavg_client_split_workspace_bytes or not device memory, FEDAVG_EALIGN
 * for one not 8-B aligned.  Nulls, sizes, codes, alignments, the table's
 * contents and the workspace's size are validated before any HIP call, and
 * everything before the first launch.
 */
int fedavg_client_chain_split_f32(float* model, float* state, const void* clients, int64_t K, int64_t D, int64_t C,
                                  int64_t rounds, int64_t step0, int activation, int optimizer, double lr, int form,
                                  const double* coef, double* losses, double* rec, void* workspace,
                                  int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTSPLIT_H */
