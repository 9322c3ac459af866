/*
 * fedavg_amd_segvec.h -- C ABI of libfedavg_amd_segvec.so: a device-resident
 * round's fp64 / fp16 / bf16 dtype group reduced straight from the clients'
 * own tensors -- the aggregate (fedavg_trainer.py:450-457) and the :291 sums
 * of squares in ONE read, no packed rows -- as fedavg_device_round_f32
 * (fedavg_amd.h) does for the fp32 group.
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_segments_vec.hip) and
 * calls no other library; fedavg_amd.h's conventions hold: device buffers
 * owned by the caller, nothing allocated inside, asynchronous and ordered on
 * `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 */
#ifndef FEDAVG_AMD_SEGVEC_H
#define FEDAVG_AMD_SEGVEC_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_segvec_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_segvec_last_error(void);

/* Bytes of host_ws (pinned) and of dev_ws (device) a round of K clients and
 * n_keys keys stages its tables in: the key table, the key-major pointer
 * table and the weights, shipped in one H2D.  0 for K <= 0 or n_keys <= 0.
 * Host arithmetic: answers without a GPU. */
int64_t fedavg_device_round_vec_workspace(int64_t K, int64_t n_keys);

/* Doubles of `partials` a round of K clients of elem_size-byte elements
 * (2 or 8; 0 for any other, and for K <= 0) needs: K x the waves of the
 * largest grid any instance launches, sized for 256 CUs; monotone in K.
 * Host arithmetic. */
int64_t fedavg_device_round_vec_partials(int64_t K, int64_t elem_size);

/* The kernel instance of K clients of elem_size bytes (is_bf16 tells the
 * 2-byte types apart): 0 = none (the call returns FEDAVG_EMODE); else
 * 3000000 + KMAX x 100 + SB as fedavg_fused_vec_plan_of encodes it, KMAX rows
 * of the instance and SB the bytes of a client's key one lane holds: a
 * window is 64 x SB / elem_size columns of one key. */
int64_t fedavg_device_round_vec_plan_of(int64_t K, int64_t elem_size, int is_bf16);

/*
 * One dtype group of a device-resident round.
 *
 * client_ptrs : [K][ptr_ld] host table of device addresses (one row per
 *               client); key j's source is column key_index[j], or column j
 *               when key_index is NULL (then ptr_ld >= n_keys).
 * key_numel / key_offset : [n_keys] elements of key j and its first element
 *               in `out`; keys may be empty, offsets are arbitrary (a key may
 *               start at any element of `out`).  Every key is raw storage of
 *               the group's dtype: there are no key kinds.
 * weights     : [K] host doubles n_i / N; rounded once to fp32 inside the
 *               call for fp16 / bf16, kept fp64 for fp64.
 * out         : device, the bits of fedavg_reduce_{f64,f16,bf16} on rows
 *               packed from the same tensors; elements outside every key are
 *               not written.
 * sumsq       : [K] device doubles, fedavg_client_sqdist_{f64,f16,bf16}'s
 *               sums by the same rounding rules, fixed order (no atomics).
 * partials    : device scratch of partial_elems >=
 *               fedavg_device_round_vec_partials(K, elem_size) doubles.
 * host_ws / dev_ws : pinned host / device scratch of ws_bytes >=
 *               fedavg_device_round_vec_workspace(K, n_keys) bytes each,
 *               16-B aligned; host_ws must stay untouched until the H2D
 *               issued on `stream` has run.
 *
 * Returns 0 (out and sumsq written; every key empty: sumsq = 0),
 * FEDAVG_EINVAL (bad sizes, null pointers, a null source of a non-empty key,
 * a workspace too small, host_ws not pinned, out / partials / sumsq / dev_ws
 * not device memory; of the sources only client 0's first and client K-1's
 * last non-empty one are checked to be device memory -- a spot check, as
 * fedavg_device_round_f32's: the caller vouches for the rest of the table),
 * FEDAVG_EALIGN (a non-empty key's source is not 16-B aligned) or
 * FEDAVG_EMODE (K beyond the one-wave bands: K > 128 for fp16 / bf16, K > 64
 * for fp64) -- all before any launch, nothing written on the device: the
 * caller packs rows then (fedavg_pack_rows_device +
 * fedavg_reduce_sqdist_{f64,f16,bf16}).  The library has no second route.
 * Sizes are validated before any HIP call.
 */
int fedavg_device_round_f64(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                            const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys,
                            int64_t K, const double* weights, double* out, double* partials,
                            int64_t partial_elems, double* sumsq, void* host_ws, void* dev_ws,
                            int64_t ws_bytes, void* stream);
int fedavg_device_round_f16(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                            const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys,
                            int64_t K, const double* weights, uint16_t* out, double* partials,
                            int64_t partial_elems, double* sumsq, void* host_ws, void* dev_ws,
                            int64_t ws_bytes, void* stream);
int fedavg_device_round_bf16(const int64_t* client_ptrs, int64_t ptr_ld, const int64_t* key_index,
                             const int64_t* key_numel, const int64_t* key_offset, int64_t n_keys,
                             int64_t K, const double* weights, uint16_t* out, double* partials,
                             int64_t partial_elems, double* sumsq, void* host_ws, void* dev_ws,
                             int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_SEGVEC_H */
