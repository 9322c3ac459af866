/*
 * fedavg_amd_fusedvec.h -- C ABI of libfedavg_amd_fusedvec.so: the aggregate
 * (fedavg_trainer.py:450-457) and the :291 sums of squares in ONE read of
 * fp64 / fp16 / bf16 client rows, as fedavg_reduce_sqdist_f32
 * (fedavg_amd.h) does for fp32 rows.
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_fused_vec.hip) and
 * links libfedavg_amd.so for the two-pass route; fedavg_amd.h's conventions
 * hold: device buffers owned by the caller, nothing allocated inside,
 * asynchronous and ordered on `stream`, 0 / FEDAVG_E* / -(hipError_t)
 * returned, K == 0 rejected.
 */
#ifndef FEDAVG_AMD_FUSEDVEC_H
#define FEDAVG_AMD_FUSEDVEC_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_fusedvec_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_fusedvec_last_error(void);

/*
 * out   : the bits of fedavg_reduce_{f64,f16,bf16}(clients, ..., weights, out);
 * sumsq : [K] doubles, fedavg_client_sqdist_{f64,f16,bf16}(clients, ..., out,
 *         ...)'s sums by the same rounding rules (the difference in the rows'
 *         dtype -- fp64, or fp32 opmath rounded to fp16 / bf16 --, squares
 *         and sum in fp64, fixed order; not necessarily the same summation
 *         tree).  Columns past P never contribute.
 * weights : [K] fp64 for fp64 rows, fp32 for fp16 / bf16 rows.
 * Rows and `out` must be 16-B aligned and ld * elem_size a multiple of 16:
 * FEDAVG_EALIGN otherwise, before any work.  Bad sizes or null pointers:
 * FEDAVG_EINVAL without touching the GPU.  P == 0 writes sumsq = 0.
 *
 * K <= 128 (fp16 / bf16) and K <= 64 (fp64) run one fused kernel: a wave
 * holds a window of 64 lanes x `slice` bytes of all K rows in registers,
 * runs the reference's chain per lane, stores the average and squares the
 * rows against it while they are still in registers.  More clients run the
 * two passes back to back inside the call.
 *
 * workspace : fedavg_reduce_sqdist_vec_workspace(K, P, elem_size) doubles of
 * device scratch (elem_size 2 or 8; 0 for any other).
 */
int64_t fedavg_reduce_sqdist_vec_workspace(int64_t K, int64_t P, int64_t elem_size);

/* The route of K x P rows of elem_size bytes (is_bf16 tells the 2-byte types
 * apart): 0 = the two passes; else kind x 1000000 + S x 100 + slots as
 * fedavg_fused_plan_of encodes it, with kind 3 (wave-owned windows), S = KMAX
 * rows of the instance and slots = the bytes of a row one lane holds. */
int64_t fedavg_fused_vec_plan_of(int64_t K, int64_t P, int64_t elem_size, int is_bf16);

int fedavg_reduce_sqdist_f64(const double* clients, int64_t K, int64_t P, int64_t ld,
                             const double* weights, double* out, double* workspace,
                             int64_t workspace_elems, double* sumsq, void* stream);
int fedavg_reduce_sqdist_f16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld,
                             const float* weights, uint16_t* out, double* workspace,
                             int64_t workspace_elems, double* sumsq, void* stream);
int fedavg_reduce_sqdist_bf16(const uint16_t* clients, int64_t K, int64_t P, int64_t ld,
                              const float* weights, uint16_t* out, double* workspace,
                              int64_t workspace_elems, double* sumsq, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_FUSEDVEC_H */
