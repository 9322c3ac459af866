/*
 * fedavg_amd_clientadam.h -- C ABI of libfedavg_amd_clientadam.so: the
 * client's Adam step (Client.train, client.py:43-44, torch.optim.Adam with
 * coupled weight decay and amsgrad=True) fused with the weight statistics of
 * client.py:76-82, in one pass over the weights, the gradients and the
 * optimizer state, for fp32, bf16, fp16 and fp64 models.
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_client_adam.hip) and
 * calls no other library; fedavg_amd.h's conventions hold: device buffers
 * owned by the caller, nothing allocated inside, asynchronous and ordered on
 * `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 *
 * Arithmetic.  T is the model's type, rT() rounds to T (nearest even); the
 * opmath type is fp32 for fp32, bf16 and fp16 and fp64 for fp64, as ATen's.
 * Every coefficient is rounded once to opmath inside the call.
 */
#ifndef FEDAVG_AMD_CLIENTADAM_H
#define FEDAVG_AMD_CLIENTADAM_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientadam_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientadam_last_error(void);

/* Elements of one unit (the 16 KiB of a weight tensor one workgroup owns) for
 * elements of elem_size bytes: 4,096 for 4, 8,192 for 2, 2,048 for 8, 0 for
 * any other.  Host arithmetic: answers without a GPU. */
int64_t fedavg_client_adam_span(int64_t elem_size);

/* Bytes of host_ws (pinned) and of dev_ws (device) the key table of n_keys
 * keys is staged in (40 per key); 0 for n_keys <= 0.  Host arithmetic. */
int64_t fedavg_client_adam_workspace(int64_t n_keys);

/* Doubles of `partials` a step over keys of key_numel[j] elements of
 * elem_size bytes needs: 3 per unit, a key of n > 0 elements being
 * ceil(n / span) units.  0 for a null table, n_keys <= 0 or an elem_size
 * other than 4, 2 and 8.  Host arithmetic. */
int64_t fedavg_client_adam_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size);

/*
 * One Adam step (torch 2.10's multi-tensor Adam, not capturable, amsgrad,
 * coupled weight decay) over a list of device tensors of type T, given as
 * HOST tables: w_ptrs[j] / g_ptrs[j] the device addresses of parameter j and
 * of its gradient (multiples of the element size), key_numel[j] their
 * elements, key_offset[j] the key's place in the state.
 *
 * state : DEVICE, 16-B aligned, 3 * state_elems elements of T: the planes
 * exp_avg (m), exp_avg_sq (v) and max_exp_avg_sq (vmax), state_elems elements
 * each (a multiple of 16 B); key j occupies [key_offset[j], key_offset[j] +
 * key_numel[j]) of every plane, key_offset[j] a multiple of 16 B.
 *
 * coef : 7 HOST doubles, formed by the caller as torch/optim/adam.py forms
 * them (t the step number from 1):
 *   coef[0] wd      coef[1] lw = 1 - beta1        coef[2] beta2
 *   coef[3] value = 1 - beta2                     coef[4] bc2s = (1 - beta2**t)**0.5
 *   coef[5] eps     coef[6] step = (lr / (1 - beta1**t)) * -1
 * Per element, every line rounded to T as the foreach op behind it stores it:
 *   A  g1    = rT(g + wd * w)              skipped entirely when wd == 0
 *   B  m'    = rT(m + lw * (g1 - m))       the difference rounded in opmath
 *      v1    = rT(v * beta2)
 *   C  v'    = rT(v1 + value * (g1 * g1))  the square rounded in opmath first
 *      vmax' = max(vmax, v')               a NaN on either side stays
 *      s1    = rT(sqrt(vmax'))
 *      s2    = rT(s1 / bc2s)               true division
 *      s3    = rT(s2 + eps)
 *   E  w'    = rT(w + step * (m' / s3))    the quotient rounded in opmath first
 *      d     = rT(w' - w)                  as `w - last_w` forms it (client.py:78)
 * then w, m, v, vmax = w', m', v', vmax' and
 *   stats[0] = the number of NaN elements of w'
 *   stats[1] = sum w'^2
 *   stats[2] = sum d^2
 *   stats[3] = 0
 * squares and sums in fp64 (exact squares of fp32 and 16-bit values, fma for
 * fp64 data), added in a fixed order (per-workgroup partials, then one
 * finalize launch; no floating-point atomics: the same bits run to run).
 *
 * form : a mask of 4 bits, one per site of the shape x + s * y (bit 0: A,
 * 1: B, 2: C, 3: E).  A set bit forms the site as one fma (one rounding in
 * opmath), a clear bit rounds product and sum apart.  Which mask equals
 * torch.optim.Adam's bits depends on how the torch build compiled its
 * kernels: the caller finds out (client_stats.adam_form).
 *
 * first != 0 : the state is all +0 and is NOT read (it is written); the
 * results equal those of first == 0 on a zeroed state bit for bit.
 *
 * Only elements [0, key_numel[j]) of each weight tensor and of each key's
 * place in the state planes are written; gradients are read only.  A side
 * (weights, gradients) of a key that is 16-B aligned is accessed 16 B at a
 * time, any other element by element, with identical results; the state is
 * always accessed 16 B at a time.  stats : 4 doubles, DEVICE, the record
 * fedavg_client_track* (fedavg_amd.h, fedavg_amd_clientvec.h) take as
 * w_stats; partials : fedavg_client_adam_partials doubles of device scratch;
 * host_ws (pinned) / dev_ws (device): fedavg_client_adam_workspace(n_keys)
 * bytes, 16-B aligned; host_ws must not be rewritten until `stream` has
 * passed the call.  n_keys == 0 (or no elements) writes stats = 0 and
 * launches nothing.  Of the coefficients only coef[1] is validated.
 *
 * Returns 0, FEDAVG_EINVAL (a negative count, null arguments, a workspace or
 * partials too small, a null tensor or one whose address is no multiple of
 * the element size, a key outside its state plane, host_ws not pinned, a
 * buffer that is not device memory), FEDAVG_EMODE (form outside 0..15, or
 * coef[1] not inside (-0.5, 0.5): Lerp.h's other branch) or FEDAVG_EALIGN (a
 * workspace, partials, stats, the state, state_elems or a key's state offset
 * misaligned).  Sizes and alignments are validated before any HIP call.
 */
int fedavg_client_adam_step_f32(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                const int64_t* key_offset, int64_t n_keys, void* state, int64_t state_elems,
                                const double* coef, int first, int form, double* partials, int64_t partial_elems,
                                double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_adam_step_bf16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                 const int64_t* key_offset, int64_t n_keys, void* state, int64_t state_elems,
                                 const double* coef, int first, int form, double* partials, int64_t partial_elems,
                                 double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_adam_step_f16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                const int64_t* key_offset, int64_t n_keys, void* state, int64_t state_elems,
                                const double* coef, int first, int form, double* partials, int64_t partial_elems,
                                double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);
int fedavg_client_adam_step_f64(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                const int64_t* key_offset, int64_t n_keys, void* state, int64_t state_elems,
                                const double* coef, int first, int form, double* partials, int64_t partial_elems,
                                double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTADAM_H */
