/*
 * fedavg_amd_clientvec.h -- C ABI of libfedavg_amd_clientvec.so: the client's
 * per-iteration statistics (Client.train, client.py:52-86) for bf16, fp16 and
 * fp64 models, as fedavg_client_stats_f32 / fedavg_client_track (fedavg_amd.h)
 * keep them for fp32 models.
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_client_vec.hip) and
 * calls no other library; fedavg_amd.h's conventions hold: device buffers
 * owned by the caller, nothing allocated inside, asynchronous and ordered on
 * `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 *
 * Arithmetic.  T is the model's type, rT() rounds to T (nearest even), f32()
 * widens exactly, fl32() rounds to fp32.  Sums of squares are fp64 sums of
 * exact squares (fp64 fma for fp64 data); a norm is the exactly rounded value
 * of what ATen's norm approximates; every scalar operation after it is done
 * as ATen does it: in opmath (fp32 for the 16-bit types), then one rounding
 * to T.
 */
#ifndef FEDAVG_AMD_CLIENTVEC_H
#define FEDAVG_AMD_CLIENTVEC_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientvec_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientvec_last_error(void);

/* Elements of one unit (the 16 KiB of a tensor one workgroup owns) for
 * elements of elem_size bytes: 8,192 for 2, 2,048 for 8, 0 for any other.
 * Host arithmetic: answers without a GPU. */
int64_t fedavg_client_stats_vec_span(int64_t elem_size);

/* Bytes of host_ws (pinned) and of dev_ws (device) the key table of n_keys
 * keys is staged in (32 per key); 0 for n_keys <= 0.  Host arithmetic. */
int64_t fedavg_client_stats_vec_workspace(int64_t n_keys);

/* Doubles of `partials` a pass over keys of key_numel[j] elements of
 * elem_size bytes needs: 3 per unit, a key of n > 0 elements being
 * ceil(n / span) units.  0 for a null table, n_keys <= 0 or an elem_size
 * other than 2 and 8.  Host arithmetic. */
int64_t fedavg_client_stats_vec_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size);

/*
 * One pass over a list of device tensors of type T (a model's params or their
 * grads), given as a HOST key table: cur_ptrs[j] the device address of tensor
 * j (a multiple of the element size), key_numel[j] its elements, key_offset[j]
 * its element offset in `snap`, a multiple of 16 bytes (8 elements of a
 * 16-bit type, 2 of fp64; FEDAVG_EALIGN otherwise).  snap : [P] elements of
 * T, DEVICE, 16-B aligned, the list as it was one step earlier.  Per element
 *   d = rT(f32(cur) - f32(snap))  for bf16 / fp16 (the difference in T, as
 *                                 `w - last_w` forms it, client.py:78, :82),
 *   d = cur - snap                for fp64,
 * and
 *   stats[0] = the number of NaN elements of cur
 *   stats[1] = sum cur^2
 *   stats[2] = sum d^2
 *   stats[3] = 0
 * squares and sums in fp64 (exact squares of the 16-bit types' values, fma
 * for fp64 data), added in a fixed order (per-workgroup partials, then one
 * finalize launch; no floating-point atomics: the same bits run to run);
 * then snap = cur, bit for bit (NaN payloads included; elements of snap
 * outside every key are not written).  has_snap == 0: snap is written only,
 * stats[2] = 0.  A 16-B aligned tensor is read with 16-B loads, any other
 * element by element, with identical results.  stats : 4 doubles, DEVICE;
 * partials : fedavg_client_stats_vec_partials doubles of device scratch;
 * host_ws (pinned) / dev_ws (device): fedavg_client_stats_vec_workspace(n_keys)
 * bytes, 16-B aligned; host_ws must not be rewritten until `stream` has
 * passed the call.  P == 0 (or no elements) writes stats = 0.
 *
 * Returns 0, FEDAVG_EINVAL (negative sizes, null arguments, a key outside the
 * snapshot, a workspace or partials too small, a null tensor or one whose
 * address is no multiple of the element size, host_ws not pinned, a buffer
 * that is not device memory) or FEDAVG_EALIGN (snap, a key offset or a
 * workspace misaligned).  Sizes and alignments are validated before any HIP
 * call.
 */
int fedavg_client_stats_bf16(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                             int64_t n_keys, uint16_t* snap, int64_t P, int has_snap, double* partials,
                             int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                             void* stream);
int fedavg_client_stats_f16(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, uint16_t* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream);
int fedavg_client_stats_f64(const int64_t* cur_ptrs, const int64_t* key_numel, const int64_t* key_offset,
                            int64_t n_keys, double* snap, int64_t P, int has_snap, double* partials,
                            int64_t partial_elems, double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes,
                            void* stream);

/*
 * The running rho / beta of client.py:78-84 kept on the device for a model of
 * type T, no host sync.  state : {rho, beta, has_rho, has_beta} doubles,
 * DEVICE, zero-initialised; rho and beta hold values of T exactly.  w_stats /
 * g_stats : this iteration's weight and gradient records; abs_dloss =
 * |loss - last_loss|, the Python double.  For bf16 / fp16, with
 * norm(S) = rT(fl32(sqrt(S))), n_w = norm(w_stats[2]), n_g = norm(g_stats[2]):
 *   rho_tmp  = rT(fl32(f32(rT(fl32(1 / f32(n_w)))) * fl32(abs_dloss)))
 *              (python_float / tensor is tensor.reciprocal() * scalar)      :78
 *   beta_tmp = rT(fl32(f32(n_g) / f32(n_w)))                                :82
 * for fp64 the same three operations in fp64 (norm(S) = sqrt(S)).  Then
 * `if not x or tmp > x: x = tmp` (:79, :83) as fedavg_client_track has it.
 */
int fedavg_client_track_bf16(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                             void* stream);
int fedavg_client_track_f16(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                            void* stream);
int fedavg_client_track_f64(double* state, const double* w_stats, const double* g_stats, double abs_dloss,
                            void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTVEC_H */
