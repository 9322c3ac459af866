/*
 * fedavg_amd_clientstep.h -- C ABI of libfedavg_amd_clientstep.so: the
 * client's plain SGD step (Client.train, client.py:74, torch.optim.SGD with
 * no momentum and no weight decay) fused with the weight statistics of
 * client.py:76-82, in one pass over the weights and the gradients, for fp32,
 * bf16, fp16 and fp64 models.
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_client_step.hip) and
 * calls no other library; fedavg_amd.h's conventions hold: device buffers
 * owned by the caller, nothing allocated inside, asynchronous and ordered on
 * `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 *
 * Arithmetic.  T is the model's type, rT() rounds to T (nearest even); the
 * opmath type is fp32 for fp32, bf16 and fp16 and fp64 for fp64, as ATen's.
 * alpha = opmath(-lr), rounded once on the host.
 */
#ifndef FEDAVG_AMD_CLIENTSTEP_H
#define FEDAVG_AMD_CLIENTSTEP_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientstep_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientstep_last_error(void);

/* Elements of one unit (the 16 KiB of a tensor one workgroup owns) for
 * elements of elem_size bytes: 4,096 for 4, 8,192 for 2, 2,048 for 8, 0 for
 * any other.  Host arithmetic: answers without a GPU. */
int64_t fedavg_client_step_span(int64_t elem_size);

/* Bytes of host_ws (pinned) and of dev_ws (device) the key table of n_keys
 * keys is staged in (32 per key); 0 for n_keys <= 0.  Host arithmetic. */
int64_t fedavg_client_step_workspace(int64_t n_keys);

/* Doubles of `partials` a step over keys of key_numel[j] elements of
 * elem_size bytes needs: 3 per unit, a key of n > 0 elements being
 * ceil(n / span) units.  0 for a null table, n_keys <= 0 or an elem_size
 * other than 4, 2 and 8.  Host arithmetic. */
int64_t fedavg_client_step_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size);

/*
 * One SGD step over a list of device tensors of type T, given as HOST tables:
 * w_ptrs[j] / g_ptrs[j] the device addresses of parameter j and of its
 * gradient (multiples of the element size), key_numel[j] their elements.
 * Per element, with w the weight before the call:
 *   form 1:  w' = rT(fma(alpha, g, w))       one rounding in opmath
 *   form 0:  w' = rT(w + fl(alpha * g))      product and sum rounded separately
 *   d  = rT(w' - w)                          the difference in T, as
 *                                            `w - last_w` forms it (client.py:78)
 * then w = w' and
 *   stats[0] = the number of NaN elements of w'
 *   stats[1] = sum w'^2
 *   stats[2] = sum d^2
 *   stats[3] = 0
 * squares and sums in fp64 (exact squares of fp32 and 16-bit values, fma for
 * fp64 data), added in a fixed order (per-workgroup partials, then one
 * finalize launch; no floating-point atomics: the same bits run to run).
 * Which form equals torch.optim.SGD's bits depends on how the torch build
 * compiled its kernel: the caller finds out (client_stats.sgd_form).  Only
 * elements [0, key_numel[j]) of each weight tensor are written; gradients are
 * read only.  A side (weights, gradients) of a key that is 16-B aligned is
 * accessed 16 B at a time, any other element by element, with identical
 * results.  stats : 4 doubles, DEVICE, the record fedavg_client_track*
 * (fedavg_amd.h, fedavg_amd_clientvec.h) take as w_stats; partials :
 * fedavg_client_step_partials doubles of device scratch; host_ws (pinned) /
 * dev_ws (device): fedavg_client_step_workspace(n_keys) bytes, 16-B aligned;
 * host_ws must not be rewritten until `stream` has passed the call.
 * n_keys == 0 (or no elements) writes stats = 0 and launches nothing.  lr is
 * not validated: torch accepts any float.
 *
 * Returns 0, FEDAVG_EINVAL (a negative count, null arguments, a workspace or
 * partials too small, a null tensor or one whose address is no multiple of
 * the element size, host_ws not pinned, a buffer that is not device memory),
 * FEDAVG_EMODE (form not 0 or 1) or FEDAVG_EALIGN (a workspace, partials or
 * stats misaligned).  Sizes and alignments are validated before any HIP call.
 */
int fedavg_client_sgd_step_f32(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_sgd_step_bf16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                                double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_sgd_step_f16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_sgd_step_f64(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                               int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                               double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTSTEP_H */
