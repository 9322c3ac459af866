/*
 * fedavg_amd_clientloop.h -- C ABI of libfedavg_amd_clientloop.so: a local
 * iteration of Client.train (client.py:69-86) that never stops the host.  The
 * :71 guard is decided on the device from the records the statistics passes
 * leave there, and the fused SGD / Adam step of fedavg_amd_clientstep.h /
 * fedavg_amd_clientadam.h runs behind that decision, its finalize launch also
 * keeping the running rho / beta of :78-84.  For fp32, bf16 and fp64 models
 * (the types the fused steps are offered for).
 *
 * The library holds its own gfx950 kernels (csrc/fedavg_client_loop.hip) and
 * calls no other library; fedavg_amd.h's conventions hold: device buffers
 * owned by the caller, nothing allocated inside, asynchronous and ordered on
 * `stream`, 0 / FEDAVG_E* / -(hipError_t) returned.
 *
 * The records, all DEVICE doubles, 8-B aligned:
 *   rec_g, rec_w : 4 doubles each, what fedavg_client_stats_* and the steps
 *                  below write: {NaN count, sum x^2, sum d^2, 0}
 *   gate         : 2 doubles {gate, trip epoch}; gate != 0: the guard tripped
 *   state        : 4 doubles {rho, beta, has rho, has beta}, as
 *                  fedavg_client_track* keep them
 *   loss         : 2 doubles {this iteration's loss, the previous one's}
 */
#ifndef FEDAVG_AMD_CLIENTLOOP_H
#define FEDAVG_AMD_CLIENTLOOP_H

#include <stdint.h>

#include "fedavg_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version of this library: bumped on any signature change. */
int fedavg_clientloop_abi_version(void);

/* Thread-local message for the last failing call of this library on this
 * thread ("" if none). */
const char* fedavg_clientloop_last_error(void);

/* Span, workspace and partials of the gated steps: the arithmetic of
 * fedavg_client_step_* (fedavg_amd_clientstep.h), and for for_adam != 0 the
 * workspace of fedavg_client_adam_workspace (40 bytes per key instead of 32).
 * Host arithmetic: they answer without a GPU. */
int64_t fedavg_client_loop_span(int64_t elem_size);
int64_t fedavg_client_loop_workspace(int64_t n_keys, int for_adam);
int64_t fedavg_client_loop_partials(const int64_t* key_numel, int64_t n_keys, int64_t elem_size);

/*
 * The :71 guard of one local iteration, decided on the device (one wave, one
 * thread working).  T is the model's type, rT() rounds to T:
 *   n_g   = norm(rec_g[1]), n_w = norm(rec_w[1])
 *           fp32: fl32(sqrt(S)); bf16: rT(fl32(sqrt(S))); fp64: sqrt(S)
 *           (sqrt the correctly rounded fp64 one; a NaN sum gives a NaN norm)
 *   bound = fp32: fl32(lr_ratio) * n_w rounded once to fp32
 *           bf16: rT of that product; fp64: n_w * lr_ratio
 *   trip  = rec_g[0] > 0 || isnan(*loss) || n_g > bound      (NaN > x is false)
 * If gate[0] == 0 and trip: gate[0] = 1, gate[1] = epoch.  A set gate is
 * never cleared and keeps its first epoch.  lr_ratio is the caller's
 * lr * THRESHOLD_GRADS_RATIO, formed in fp64.
 *
 * Returns 0, FEDAVG_EINVAL (a null argument, a negative epoch, a record that
 * is not device memory) or FEDAVG_EALIGN (a record not 8-B aligned).  Null,
 * sign and alignment are validated before any HIP call.
 */
int fedavg_client_guard_f32(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                            double lr_ratio, int64_t epoch, void* stream);
int fedavg_client_guard_bf16(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                             double lr_ratio, int64_t epoch, void* stream);
int fedavg_client_guard_f64(const double* rec_g, const double* rec_w, const double* loss, double* gate,
                            double lr_ratio, int64_t epoch, void* stream);

/*
 * fedavg_client_sgd_step_* (fedavg_amd_clientstep.h) behind the gate, with the
 * track update in its finalize launch.  The first thirteen arguments are that
 * entry's, with its forms, checks and bits; `stats` is the weight record
 * rec_w.  Then:
 *   g_stats : the gradient record rec_g (read: sum d^2 for beta)
 *   gate    : read by every workgroup of both launches before anything else
 *   state   : the running rho / beta
 *   loss    : the two loss slots
 * gate[0] != 0: both launches return at once and write NOTHING: the weights,
 * partials, stats, state and both loss slots keep their bits.  gate[0] == 0:
 * the step and its record exactly as fedavg_client_sgd_step_* leave them; the
 * finalize launch then does what fedavg_client_track* does with
 * abs_dloss = |loss[0] - loss[1]| (formed in fp64) and sets loss[1] = loss[0].
 * n_keys == 0 (or no elements): no step launch; the finalize launch writes
 * stats = 0 and the track update, behind the gate like any other.
 *
 * Returns what fedavg_client_sgd_step_* returns, and FEDAVG_EINVAL for a null
 * g_stats, gate, state or loss or one that is not device memory, FEDAVG_EALIGN
 * for one that is not 8-B aligned.  Sizes, nulls and alignments are validated
 * before any HIP call.
 */
int fedavg_client_sgd_step_gated_f32(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                     int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                                     double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream,
                                     const double* g_stats, const double* gate, double* state, double* loss);
int fedavg_client_sgd_step_gated_bf16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                      int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                                      double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream,
                                      const double* g_stats, const double* gate, double* state, double* loss);
int fedavg_client_sgd_step_gated_f64(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                     int64_t n_keys, double lr, int form, double* partials, int64_t partial_elems,
                                     double* stats, void* host_ws, void* dev_ws, int64_t ws_bytes, void* stream,
                                     const double* g_stats, const double* gate, double* state, double* loss);

/*
 * fedavg_client_adam_step_* (fedavg_amd_clientadam.h) behind the gate in the
 * same way: the first seventeen arguments are that entry's (`state` there is
 * the optimizer state `adam_state` here), then the four above.  A set gate
 * also leaves the three state planes as they were.
 */
int fedavg_client_adam_step_gated_f32(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                      const int64_t* key_offset, int64_t n_keys, void* adam_state,
                                      int64_t state_elems, const double* coef, int first, int form, double* partials,
                                      int64_t partial_elems, double* stats, void* host_ws, void* dev_ws,
                                      int64_t ws_bytes, void* stream, const double* g_stats, const double* gate,
                                      double* state, double* loss);
int fedavg_client_adam_step_gated_bf16(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                       const int64_t* key_offset, int64_t n_keys, void* adam_state,
                                       int64_t state_elems, const double* coef, int first, int form, double* partials,
                                       int64_t partial_elems, double* stats, void* host_ws, void* dev_ws,
                                       int64_t ws_bytes, void* stream, const double* g_stats, const double* gate,
                                       double* state, double* loss);
int fedavg_client_adam_step_gated_f64(const int64_t* w_ptrs, const int64_t* g_ptrs, const int64_t* key_numel,
                                      const int64_t* key_offset, int64_t n_keys, void* adam_state,
                                      int64_t state_elems, const double* coef, int first, int form, double* partials,
                                      int64_t partial_elems, double* stats, void* host_ws, void* dev_ws,
                                      int64_t ws_bytes, void* stream, const double* g_stats, const double* gate,
                                      double* state, double* loss);

#ifdef __cplusplus
}
#endif

#endif /* FEDAVG_AMD_CLIENTLOOP_H */
