/*
 * fedavg_amd_clientwide.h -- C ABI of libfedavg_amd_clientwide.so: the local
 * loops of ALL the linear clients of a round (fedavg_trainer.py:172-199) for
 * MODELS OF UP TO 128 CLASSES AND 4096 COLUMNS
 * (csrc/fedavg_client_wide.hip).  The contract is that of
 * fedavg_client_cohort_split_f32 (fedavg_amd_clientcosplit.h) with wider
 * ranges: every client trained from the same model for `iters` local
 * iterations under the :71 guard, client `row` into row `row` of the packed
 * buffer the reduce reads, one record of eight fields per client.  fp32 model,
 * fp32 batches, int64 labels.
 *
 * The other linear libraries admit one 16-wide class tile and 1024 columns;
 * this one tiles classes (CT = ceil(C / 16) tiles) and columns (panels of 128)
 * and spreads the step over workgroups.  A call is one setup launch and FOUR
 * launches per local iteration, enqueued back to back on `stream` with no
 * host sync, no atomic and no grid barrier:
 *   setup    : once, as the cosplit library's.  With R = 64 rows a slice,
 *              G_k = ceil(B_k / R) and q = slices_per_group, client k has
 *              n_k = ceil(G_k / q) workgroups and workgroup j of it owns
 *              slices [j q, min((j + 1) q, G_k)).
 *   gradient : sum_k n_k workgroups of 512 threads.  x streams in units of
 *              64 rows x 128 columns through two LDS buffers (rows of 132
 *              floats), the next unit requested before the current one is
 *              consumed; a workgroup never holds a full row.  Forward, slice
 *              by slice and panel by panel: each (row tile, class tile)
 *              product of z = x W^T belongs to one wave for the whole of D
 *              and accumulates in its registers on the 16x16x4 fp32 matrix
 *              instruction, W read from the client's row.  With C <= 16 four
 *              of the eight waves have no product.  z goes to an LDS store of
 *              q x 64 rows of 16 CT + 1 floats (one float of padding: the
 *              rows of the per-sample pass on different banks).  Per-sample:
 *              one thread per row walks its C logits in class order (bias,
 *              optional sigmoid, log-softmax, loss term, argmax with
 *              first-index ties) and overwrites z with dz; thread 0 adds the
 *              loss terms (fp64) and the correct counts, thread c column c of
 *              dz, in sample order.  Backward, panel by panel and slice by
 *              slice: the units stream a second time and a panel's dW tiles
 *              accumulate dz^T x over the group's slices in slice order; each
 *              is written once to the workgroup's slot of the plane.
 *   sum      : grid (ceil(P / 8192) chunks, K).  The client's n_k slots are
 *              added in slot order into this epoch's gradient; per chunk the
 *              sums of g^2, (g - last_g)^2, w^2 and the NaN count.
 *   step     : the same grid.  Every workgroup adds its client's chunk
 *              partials in chunk order in fp64 and so reaches the same
 *              verdict on the guard; it applies the SGD or Adam element rule
 *              to its chunk of the row (Adam's m, v, vmax in the workspace)
 *              and writes its partial of sum (w' - w)^2.
 *   track    : one workgroup per client: the same verdict; rho / beta, the
 *              last loss, the trip, the record.
 * last_grads is the gradient block of the epoch before: the two blocks change
 * roles every epoch.  A client with a bad label or a tripped guard is inert
 * for the rest of the call: its workgroups return at once in every launch.
 * The kernels use no scratch memory.
 *
 * Bit contract:
 *   - row k and record k are a function of client k's inputs, `model`, the
 *     hyper-parameters and slices_per_group alone: they do not depend on the
 *     other clients, on the table's order or on K;
 *   - two calls on equal inputs leave equal bits;
 *   - the results are NOT the bits of fedavg_client_cohort_f32 or
 *     fedavg_client_cohort_split_f32 where the shapes overlap: the logits'
 *     columns, the gradient's slots and the guard's sums are added in another
 *     (fixed) order here;
 *   - nothing past workspace_bytes is touched and columns [P, ld) of a row
 *     are not written.
 * The element rules, the guard and the rho / beta track are those of the
 * other client libraries (csrc/client_step_rules.hpp, client_adam_rules.hpp,
 * client_pass.hpp).
 *
 * The library calls no other library; fedavg_amd.h's conventions hold:
 * buffers owned by the caller, nothing allocated inside, asynchronous and
 * ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_CLIENTWIDE_H
#define FEDAVG_AMD_CLIENTWIDE_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientwide_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientwide_last_error(void);

/* The ranges: K <= 4096 clients, 1 <= B <= 16384 rows, 1 <= D <= 4096
 * columns, 2 <= C <= 128 classes, P = C * D + C <= 128 * 4097.  A null
 * pointer is skipped. */
void fedavg_client_wide_limits(int64_t* max_k, int64_t* max_b, int64_t* max_d, int64_t* max_c, int64_t* max_p);

/* R, the rows of a slice: 64 at every shape. */
int64_t fedavg_client_wide_slice_rows(void);

/* The largest slices_per_group at C classes: the most slices whose dz store
 * (64 * (16 * ceil(C / 16) + 1) * 4 bytes each) fits beside the two unit
 * buffers (2 * 64 * 132 * 4 bytes) inside the LDS budget
 * fedavg_client_stream_limits reports (132864 bytes), and at most 15: 15 up
 * to C = 16, 3 at C = 62, 1 at C = 128.  0 for C outside [2, 128]. */
int64_t fedavg_client_wide_max_slices(int64_t C);

/* The bytes of workspace a call needs for clients of B[0 .. K) rows.  With
 * N = sum_k n_k (above), P = C * D + C, NC = ceil(P / 8192) and a = 1 for
 * Adam (optimizer 1), 0 for SGD (optimizer 0):
 *     104 K + 24 N + 40 K NC + 4 P (N + K (2 + 3 a))
 * per client its table entry (32), its state block (64) and its span of slots
 * (8), per workgroup its group entry (8), its loss sum and correct count (16)
 * and its slot of the plane (4 P), per client and chunk the sum launch's four
 * partials (32) and the step launch's one (8), per client the two gradient
 * blocks (8 P) and Adam's m, v, vmax (12 P).  0 for a null B, K outside
 * [1, 4096], a B[k] outside [1, 16384], D outside [1, 4096], C outside
 * [2, 128], slices_per_group outside [1, fedavg_client_wide_max_slices(C)] or
 * an optimizer that is neither.  Host arithmetic. */
int64_t fedavg_client_wide_workspace_bytes(const int64_t* B, int64_t K, int64_t D, int64_t C,
                                           int64_t slices_per_group, int optimizer);

/*
 * The cohort at the wider shapes.  Every argument is that of
 * fedavg_client_cohort_split_f32, in its order: model, rows, ld, clients (the
 * 32-B pinned entries {x, y, B, row}, `row` a permutation of 0 .. K - 1), K,
 * D, C, iters, activation, optimizer, lr, lr_ratio, form, coef, rec ([K, 8]:
 * trip epoch or -1, loss, beta, rho, correct count, label flag, steps taken,
 * 0), slices_per_group, workspace, workspace_bytes, stream; the ranges are
 * those of fedavg_client_wide_limits.
 *   slices_per_group: 1 <= q <= fedavg_client_wide_max_slices(C)
 *   workspace       : device memory, 8-B aligned, of `workspace_bytes` bytes,
 *                     at least fedavg_client_wide_workspace_bytes(the table's
 *                     B, K, D, C, slices_per_group, optimizer); its contents
 *                     on entry do not matter
 * The call enqueues 1 + 4 * iters launches.  A client with a label outside
 * [0, C) gets label flag 1 and a copy of `model` in its row and touches no
 * other client; a client whose guard trips keeps in its row the parameters at
 * the trip.  Units go from global memory straight into LDS when D % 4 == 0
 * and every x is 16-B aligned, otherwise every unit is staged through
 * registers; the bits do not depend on which.  Loss and correct count are the
 * last epoch's, from before its step.
 *
 * Returns what fedavg_client_cohort_split_f32 returns for the same arguments,
 * in the same order of checks, with FEDAVG_EINVAL for a P above 128 * 4097
 * (after C) and for a slices_per_group outside its range (where that entry
 * refuses one below 1); the message names the value and the range.  Nulls,
 * sizes, codes, alignments, the table's contents and the workspace's size are
 * validated before any HIP call, and everything before the first launch.
 */
int fedavg_client_cohort_wide_f32(const float* model, float* rows, int64_t ld, const void* clients, int64_t K,
                                  int64_t D, int64_t C, int64_t iters, int activation, int optimizer, double lr,
                                  double lr_ratio, int form, const double* coef, double* rec,
                                  int64_t slices_per_group, void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTWIDE_H */
