/*
 * nmfx.h -- C ABI of the MI355X-native NMF solver engine (libnmfx.so).
 *
 * The reference (raleng/nmf) is pure Python and has no FFI of its own; its
 * boundary is the Python call surface NMF(data, k).factorize(method=...) and the
 * four solver functions it forwards to.  This header is the native boundary a
 * maintainer would bind (ctypes stub in INTEGRATION.md) to replace the bodies of
 * those solver loops.  Each entry point names the reference lines it replaces
 * (paths relative to the reference checkout).
 *
 * Conventions
 *  - plain C, opaque handle, plain pointers and sizes; no torch / numpy types.
 *  - host matrices are C-contiguous row-major like the reference's ndarrays.
 *    Factors cross the boundary as float64 (the reference's dtype for W/H,
 *    nmf/utils.py:51-52); the engine computes in float32 on MFMA and keeps
 *    objective sums in float64.
 *  - every function returns 0 or a negative NMFX_E_* code; nmfx_last_error()
 *    gives the message.  One handle = one device + one stream; a handle is not
 *    thread-safe, independent handles are.
 *  - the caller owns all host buffers, the library owns all device buffers
 *    (except exchange buffers handed in with nmfx_set_exchange_buffers).
 *  - device-side control flow: a stop flag in device memory is set by the
 *    engine when the reference's convergence_check (nmf/utils.py:4-15) fires;
 *    all later launches become no-ops, so iterations can be queued in batches
 *    without a host round trip per iteration.
 */
#ifndef NMFX_H
#define NMFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nmfx_engine* nmfx_handle_t;

enum {
    NMFX_OK = 0,
    NMFX_E_ARG = -1,     /* bad argument / unsupported request (k > 128 in a row-sharded AO-ADMM / ADMM / ANLS phase) */
    NMFX_E_HIP = -2,     /* HIP runtime error, no device                          */
    NMFX_E_NOTPD = -3,   /* Gram + rho I not positive definite (scipy LinAlgError, nmf/ao_admm.py:55) */
    NMFX_E_STATE = -4,   /* call sequence error (no V uploaded, no factors set)   */
    NMFX_E_NOMEM = -5,
    NMFX_E_RCCL = -6     /* RCCL not found (dlopen) or a collective / communicator call failed */
};

enum { NMFX_F32 = 0, NMFX_F64 = 1 };                 /* host dtype of V          */
enum { NMFX_EU = 0, NMFX_KL = 1, NMFX_IS = 2, NMFX_BETA = 3 };      /* distance_type (IS, BETA: nmfx_mur_run / nmfx_mur_finish only) */
enum { NMFX_PROX_NN = 0, NMFX_PROX_L1N = 1, NMFX_PROX_L2N = 2,      /* reg type   */
       NMFX_PROX_L1INF = 3, NMFX_PROX_L1INF_T = 4 };                /* ADMM only (nmf/admm.py:158-210) */

/* ---- lifecycle ---------------------------------------------------------- */
/* m, n: rows/cols of the LOCAL block of V held by this handle (all of V on one
 * GPU; a row shard when the caller shards rows over ranks).  k <= 4096 (nmf/nmf.py:32-35 accepts any `factors`): up to 128
 * every solver runs its tuned kernels; beyond that (padded to a multiple of 128) the MUR entry points and the whole-loop
 * entry points nmfx_aoadmm_run / nmfx_admm_run / nmfx_anls_run compose their iterations from a generic exact-f32 product
 * kernel (kernels_generic.hip); the row-sharded phase entry points of AO-ADMM / ADMM / ANLS stay at k <= 128.  HALS runs
 * up to 128 components through nmfx_hals_run and from 129 to 1024 through nmfx_hals_wide_run (version 396); its sparse, masked,
 * stacked and fold-in forms stay at the ranks their sections name. */
int nmfx_create(nmfx_handle_t* out, int device, int64_t m, int64_t n, int k);
int nmfx_destroy(nmfx_handle_t h);
const char* nmfx_last_error(nmfx_handle_t h);        /* h may be NULL            */
int nmfx_version(void);
int nmfx_device_count(void);
/* Run on a caller-provided hipStream_t (e.g. torch's current stream) instead of
 * the handle's own non-blocking stream.  NULL is HIP's default (null) stream --
 * which is what torch.cuda.current_stream() is unless the caller changed it.
 * nmfx_reset_stream goes back to the handle's own stream.                      */
int nmfx_set_stream(nmfx_handle_t h, void* hip_stream);
int nmfx_reset_stream(nmfx_handle_t h);
int nmfx_synchronize(nmfx_handle_t h);
/* Arithmetic of the V-sized products: 0 = f32-input MFMA (exact
 * f32 FMA chains), 1 = split bf16 (each f32 operand as bf16 hi + bf16 lo, three or four
 * bf16 MFMA terms per product -- kernels_bf16.hip, top -- f32 accumulation; available when
 * k pads to 64 or 128, otherwise mode 0 is used; every solver's Euclidean products and
 * MUR-KL's quotient products).  nmfx_get_precision returns the mode in effect.
 * Environment override at create time: NMFX_PRECISION=f32|bf16.                 */
int nmfx_set_precision(nmfx_handle_t h, int mode);
int nmfx_get_precision(nmfx_handle_t h);
/* What nmfx_create decided on its own, in words ("" if nothing): today the fall back to the exact-f32 kernels when the
 * two extra V-sized buffers of the split-bf16 path do not fit into the free device memory.  (In split-bf16 mode the
 * row-major copy of a V of 4 GiB or more is freed once the tile-major copies exist -- NMFX_DROP_V=0/1 overrides -- and
 * rebuilt when a kernel needs it.)                                                                                  */
const char* nmfx_get_note(nmfx_handle_t h);

/* ---- data --------------------------------------------------------------- */
/* Copy rows [row0, row0+rows) of the local V from host memory (row stride `ld`
 * elements, dtype NMFX_F32/F64).  V is borrowed, never modified (the MUR shift
 * of negative data, nmf/mur.py:99-101, is done by the caller on its array).   */
int nmfx_upload_v(nmfx_handle_t h, const void* host, int dtype, int64_t ld,
                  int64_t row0, int64_t rows);
/* The same from DEVICE memory of the handle's GPU (a block the caller produced there, e.g. a
 * torch tensor's data_ptr): device-to-device copy into the engine's padded layout, no PCIe.
 * The caller makes sure the producer of `dev` has finished (the copy runs on the handle's
 * stream); the call returns when the copy is done, `dev` may then be freed.                 */
int nmfx_upload_v_device(nmfx_handle_t h, const void* dev, int dtype, int64_t ld,
                         int64_t row0, int64_t rows);
/* ---- per-entry weights (version 340) ---------------------------------------
 * Omega >= 0 with the shape of the local V, conventions of nmfx_upload_v (rows [row0, row0 + rows), row stride `ld`, dtype
 * NMFX_F32 / F64, stored as f32).  A cell with weight 0 is unknown, not zero: V is not part of any sum there.  The buffer
 * (the size of V) is allocated zeroed by the first call, so rows never uploaded carry zero weight; NMFX_E_NOMEM with a
 * message when it does not fit.  Legal on a dense handle with k <= 128: NMFX_E_ARG on a sparse handle and for k > 128,
 * nothing launched.  The entries must be finite and >= 0 (not checked here).
 * While weights are present nmfx_mur_run / nmfx_mur_finish with NMFX_EU, NMFX_KL or NMFX_IS run the weighted update
 * (kernels_phase.hip, exact f32 whatever the precision mode; nmfx_get_note says so), with T = W H and W' the new W:
 *   Euclidean  W <- W ((Om.V) H^T) / ((Om.T) H^T + lambda_w W + 1e-9)                          1/2 Sum om (v - T)^2
 *   KL         A = W ((Om.V / (T + 1e-9)) H^T),  B = Om H^T,  W <- 2 A / (B + sqrt(B^2 + 4 lambda_w A)),  0 where B = 0
 *                                                                                              Sum om [v log(v / T) - v + T]
 *   IS         q = T + 1e-9,  W <- W sqrt( ((Om.V / q^2) H^T) / ((Om / q) H^T + lambda_w) ),  0 where the denominator is 0
 *                                                                                              Sum om [v / q - log(v / q) - 1]
 *   H likewise with W' and lambda_h; the objective is recorded in f64 with the iteration contract of nmfx_mur_run.
 * nmfx_set_factors, nmfx_get_factors, nmfx_get_state, nmfx_get_objectives, nmfx_set_stop_guard, nmfx_resume,
 * nmfx_set_stream, nmfx_reset_stream, nmfx_synchronize and nmfx_destroy keep their meaning, as do the entry points that
 * only move data or read settings.  Every other compute entry point -- the MUR phase / chunk / slice / sharded forms,
 * pair mode, nmfx_objective_f64, nmfx_profile_repeat, AO-ADMM, ADMM, ANLS, nmfx_topk_svd -- returns NMFX_E_ARG with a
 * message naming the weights and launches nothing.  nmfx_clear_weights frees the buffer: the handle behaves as before. */
int nmfx_upload_weights(nmfx_handle_t h, const void* host, int dtype, int64_t ld, int64_t row0, int64_t rows);
int nmfx_clear_weights(nmfx_handle_t h);
/* ---- the beta-divergence (version 350) -------------------------------------
 * nmfx_set_beta stores beta on the handle for runs with distance = NMFX_BETA (the reference has no such loss).  Legal on a
 * dense handle with k <= 128 and -1 <= beta <= 3: NMFX_E_ARG for a beta outside that range (NaN included), on a sparse
 * handle and for k > 128; nothing is launched and a beta stored before stays.  The range is what f32 carries: a cell can
 * have q = 1e-9, and q^(beta - 2) times v has to stay finite.
 * nmfx_mur_run / nmfx_mur_finish then accept NMFX_BETA (NMFX_E_STATE if beta was never set), with or without the weights
 * of nmfx_upload_weights (Om = 1 without).  q = W H + 1e-9, W' the new W:
 *   gamma = 1 / (2 - beta) for beta < 1,  1 for 1 <= beta <= 2,  1 / (beta - 1) for beta > 2
 *   W <- W ( ((Om.V.q^(beta-2)) H^T) / ((Om.q^(beta-1)) H^T + lambda_w) )^gamma,  H likewise with W' and lambda_h,
 *   0 where the denominator is 0  (the MM rule of Fevotte & Idier 2011)
 *   objective  Sum om d_beta(v | q),  d_beta = (v^beta + (beta-1) q^beta - beta v q^(beta-1)) / (beta (beta-1)),
 *              v log(v / q) - v + q at beta = 1 (log term 0 at v = 0),  v / q - log(v / q) - 1 at beta = 0,
 *   recorded in f64 with the iteration contract of nmfx_mur_run.  For beta <= 0 V must be strictly positive
 *   wherever it is part of the fit; for beta > 0 a zero is data (not checked here).  beta = 0, 1, 2 run this general rule:
 *   NMFX_IS, NMFX_KL and NMFX_EU keep their own kernels and results.
 * The kernels (kernels_phase.hip) are exact f32 whatever the precision mode; nmfx_get_note says so once a beta is set.
 * Every entry point that refuses NMFX_IS -- the MUR phase / chunk / slice / sharded forms, nmfx_profile_repeat -- refuses
 * NMFX_BETA the same way: NMFX_E_ARG, a message naming beta, nothing launched; so does nmfx_objective_f64 (a Euclidean
 * objective) on a handle whose current run is a beta run. */
int nmfx_set_beta(nmfx_handle_t h, double beta);
/* ---- automatic relevance determination (version 360) -----------------------
 * The l1 form of Tan & Fevotte (TPAMI 2013) on top of the beta-divergence: component c < k of a run with k chosen too large
 * carries a relevance lambda_c shared by column c of W and row c of H, and the superfluous components are driven to zero
 * during the run.  With F x N the shape of the local V, phi > 0 the dispersion, a > 0, b > 0 and c = F + N + a + 1:
 *   C(W, H, lambda) = Sum om d_beta(v | q)  +  phi Sum_{c<k} [ (|w_c|_1 + |h_c|_1 + b) / lambda_c + c log lambda_c ]
 *   lambda_c = (|w_c|_1 + |h_c|_1 + b) / c          (the closed-form minimiser; its floor is b / c)
 *   W <- W ( ((Om.V.q^(beta-2)) H^T) / ((Om.q^(beta-1)) H^T + phi / lambda_c) )^gamma       column c uses phi / lambda_c
 *   H likewise with W' and the same lambda (row c uses phi / lambda_c); then lambda is recomputed from the new pair.
 * nmfx_set_ard turns it on: a dense handle with k <= 128 on which a beta is set.  NMFX_E_ARG for a parameter that is not
 * finite or not > 0, on a sparse handle and for k > 128; NMFX_E_STATE when no beta is set; nothing is launched.  While it is
 * set, nmfx_mur_run / nmfx_mur_finish accept only NMFX_BETA with lambda_w = lambda_h = 0 (NMFX_E_ARG otherwise) and record
 * obj[j] = C(W_j, H_j, lambda_j) = Sum om d_beta + phi c Sum_{c<k} (1 + log lambda_c), both parts and their sum in f64, under
 * the usual stop rule; lambda_0 is computed from the start factors at the first run after nmfx_set_factors.  Every other
 * compute entry point -- the MUR phase / chunk / slice / sharded forms, pair mode, nmfx_profile_repeat, AO-ADMM, ADMM, ANLS,
 * nmfx_topk_svd -- returns NMFX_E_STATE and launches nothing.  nmfx_set_beta keeps ARD set (the relevances are recomputed
 * before the next run).  nmfx_clear_ard turns it off: a run then equals a fresh handle's bit for bit.
 * nmfx_get_relevance copies lambda_c, c < k, of the current iterate -- the one nmfx_get_factors returns -- to lambda_out
 * (NMFX_E_STATE without nmfx_set_ard or factors).  The sums are f64 over the f32 factors in a fixed order. */
int nmfx_set_ard(nmfx_handle_t h, double phi, double a, double b);
int nmfx_clear_ard(nmfx_handle_t h);
int nmfx_get_relevance(nmfx_handle_t h, double* lambda_out /* k */);
/* ---- sparse V (version 310) ----------------------------------------------
 * A handle for a sparse m x n V with `nnz` stored entries, 1 <= k <= 256.  It runs MUR (both losses) without ever
 * forming V densely: nmfx_upload_csr takes V as CSR -- row_ptr [m + 1] (int64: nnz may pass 2^31), col_idx [nnz]
 * strictly increasing within each row (no duplicates), values [nnz] >= 0 in dtype NMFX_F32 / NMFX_F64, stored as f32 --
 * and builds the transposed (CSC) index itself, deterministically.  The arrays are borrowed, never modified.
 * On a sparse handle these entry points keep their meaning and the iteration contract of a dense handle, with the same
 * layouts of W and H: nmfx_set_factors, nmfx_get_factors, nmfx_mur_run, nmfx_mur_finish, nmfx_get_state,
 * nmfx_get_objectives, nmfx_objective_f64, nmfx_set_stop_guard, nmfx_resume, nmfx_synchronize, nmfx_set_stream
 * (and nmfx_reset_stream, nmfx_destroy, nmfx_last_error, nmfx_get_note; from version 391 nmfx_profile_enable,
 * nmfx_profile_get and nmfx_profile_reset, which count the sp_* scopes, and nmfx_hals_sparse_run / _finish on an unmasked
 * handle with k <= 128; from version 392 nmfx_hals_masked_run / _finish on a masked handle with k <= 64; from version 393 nmfx_hals_foldin_run and
 * nmfx_hals_foldin_get_sweeps on either; from version 397 nmfx_hals_sparse_wide_run / _finish on an unmasked handle with 128 < k <= 256).  The objective is recorded in f64 from the non-zeros plus k x k terms ("Sparse V").
 * Every other entry point returns NMFX_E_ARG and launches nothing. */
int nmfx_create_csr(nmfx_handle_t* out, int device, int64_t m, int64_t n, int k, int64_t nnz);
int nmfx_upload_csr(nmfx_handle_t h, const int64_t* row_ptr, const int32_t* col_idx, const void* values, int dtype);
/* Masked V (version 320).  on = 1: the stored entries are the OBSERVED set M -- stored zeros included -- and every other
 * entry is unknown, not zero.  Legal only between nmfx_create_csr and nmfx_upload_csr (NMFX_E_ARG on a dense handle,
 * NMFX_E_STATE after the upload; neither launches anything).  MUR then runs the weighted (0/1) Lee-Seung update
 *   Euclidean  W <- W (M.X) H^T / ((M.(W H)) H^T + lambda_w W + 1e-9),  H likewise with the new W
 *   KL         A = W ((M.X / (W H + 1e-9)) H^T),  B = M H^T,  W <- 2 A / (B + sqrt(B^2 + 4 lambda_w A)),  0 where B = 0
 * and records Sum_M 1/2 (x - wh)^2 (Euclidean) / Sum_M [x log(x / wh) - x + wh] (KL) in f64 ("Masked V").
 * The other entry points keep the sparse handle's contract; nmfx_objective_f64 gives the masked Euclidean objective. */
int nmfx_set_masked(nmfx_handle_t h, int on);

/* W (m x k) and H (k x n), float64 row-major; either may be NULL to skip.
 * set_factors also zeroes all dual/auxiliary state and the iteration state.   */
int nmfx_set_factors(nmfx_handle_t h, const double* w, const double* hmat);
int nmfx_get_factors(nmfx_handle_t h, double* w, double* hmat);
/* Other state matrices by name: "dual_w" "dual_h" (AO-ADMM / ADMM),
 * "w_aux" "h_aux" (ADMM).  Shapes as W / H.                                   */
int nmfx_get_matrix(nmfx_handle_t h, const char* name, double* out);
/* The inverse: overwrite one of those state matrices (allocates the ADMM state on first use). */
int nmfx_set_matrix(nmfx_handle_t h, const char* name, const double* in);

/* ---- iteration state ---------------------------------------------------- */
/* stop_rule: 0 running, 1 / 2 = which branch of convergence_check fired
 * (nmf/utils.py:8-11); stop_i: the reference's loop index `i` at which it
 * fired; n_obj: number of objective values recorded so far (obj[0] is the
 * objective of the initial factors, nmf/mur.py:115).                           */
int nmfx_get_state(nmfx_handle_t h, int* stop_rule, int64_t* stop_i, int64_t* n_obj);
int nmfx_get_objectives(nmfx_handle_t h, int64_t first, int64_t count, double* out);
/* NNLS diagnostics of ANLS since the last nmfx_set_factors: passive variables dropped because their pivot vanished
 * (a dead or collinear component at lambda = 0; their x stays 0 like in scipy's nnls / nmf/fcnnls.py) and solves that
 * ran into the iteration cap (8 k + 64 exchanges; the reference's FCNNLS prints 'Not converged.' in that case).      */
int nmfx_get_diagnostics(nmfx_handle_t h, int64_t* nnls_evicted, int64_t* nnls_capped);
/* How often the default NNLS path (f64 inverse of the Gram matrix + complement of the passive set) handed work
 * to the elimination kernels since the last nmfx_set_factors: single problems (complement larger than its workspace), and whole
 * half-steps (Gram matrix singular or too ill-conditioned for an explicit inverse).                                         */
int nmfx_get_nnls_fallbacks(nmfx_handle_t h, int64_t* problems, int64_t* half_steps);
/* AO-ADMM, fused inner rounds (nmf/ao_admm.py:58-66 run speculatively, DESIGN.md 4b "hinted speculation"): how many
 * sub-problems since the last nmfx_set_factors had a first leg that [0] stood as it was, [1] was cut back to an earlier round, [2] had to be
 * continued to admm_iter, [3] was continued and then cut back.  Cost diagnostics only: the rounds that count and their
 * arithmetic are the reference's on every path.                                                                          */
int nmfx_get_inner_paths(nmfx_handle_t h, int64_t out[4]);

/* ---- MUR (replaces the loop body nmf/mur.py:119-131) -------------------- */
/* Queue `count` outer iterations starting at iteration `first` (= number of
 * iterations already run on this handle).  Iteration j computes, like
 * mur.py:122-127: W <- w_update (mur.py:20-33), H <- h_update with the new W
 * (mur.py:36-49), objective of the result (utils.py:18-33), and the
 * convergence check for `i = j` when j > min_iter (mur.py:131).  Asynchronous;
 * read results with nmfx_get_state / nmfx_get_objectives (they synchronise).
 * distance = NMFX_IS (version 330; the reference has no such loss): the Itakura-Saito divergence, with q = W H + 1e-9,
 *   W <- W sqrt( ((V / q^2) H^T) / ((1 / q) H^T + lambda_w) ),  H likewise with the new W,  0 where the denominator is 0,
 *   objective Sum [v / q - log(v / q) - 1] in f64 ("Itakura-Saito").  V must be strictly positive where it is
 *   part of the fit.  Accepted by nmfx_mur_run and nmfx_mur_finish alone, on a dense handle with k <= 128 (exact-f32
 *   kernels whatever the precision mode; nmfx_get_note says so) and on a masked sparse handle (sums over the observed
 *   set).  An unmasked sparse handle (its zeros have infinite IS divergence), k > 128 on a dense handle, the phase /
 *   chunk / slice / sharded entry points and nmfx_profile_repeat return NMFX_E_ARG with a message naming IS and launch
 *   nothing, as does nmfx_objective_f64 (a Euclidean objective) on a handle whose current run is an IS run.            */
int nmfx_mur_run(nmfx_handle_t h, int distance, double lambda_w, double lambda_h,
                 int64_t min_iter, double tol1, double tol2,
                 int64_t first, int64_t count);
/* Complete the objective/convergence bookkeeping of the last queued iteration
 * (the engine evaluates the objective of iteration j inside the first kernel
 * of iteration j+1; this runs that evaluation alone).                         */
int nmfx_mur_finish(nmfx_handle_t h, int distance, int64_t min_iter, double tol1,
                    double tol2, int64_t iters_done);

/* ---- fold-in (version 370): H for new data against a fixed W -----------------
 * The reference has nothing of the kind.  After nmfx_upload_v (the new data) and nmfx_set_factors(w, h0), iteration j applies
 * the H half-step of nmfx_mur_run for the same loss and W is never updated:
 *   NMFX_EU    H <- H (W^T V) / (W^T (W H) + lambda_h H + 1e-9)                          (nmf/mur.py:36-49 with w fixed)
 *   NMFX_KL    A = H (W^T (V / (W H + 1e-9))),  B = W^T 1,  H <- 2 A / (B + sqrt(B^2 + 4 lambda_h A)),  0 where B = 0
 *   NMFX_IS, NMFX_BETA (after nmfx_set_beta), and every loss with the weights of nmfx_upload_weights: the H step stated at
 *   nmfx_mur_run, nmfx_upload_weights and nmfx_set_beta, a zero denominator gives 0.
 * obj[j] is the objective of (W, H_j), obj[0] that of the start h0, recorded in f64 with the iteration contract and the stop
 * rule of nmfx_mur_run (`first` = iterations already run; nmfx_foldin_finish records the objective of the last pair).  One
 * step is ONE pass over V: the H phase also sums the objective of the pair it starts from (kernels_phase.hip).
 * V is never modified; two runs are bit-identical.  Legal on a dense handle with k <= 128; the kernels are exact f32
 * whatever the precision mode and nmfx_get_note says so after the first call.  Refused, with a message and nothing launched:
 * a sparse handle, k > 128 and an unknown distance (NMFX_E_ARG); NMFX_BETA without a beta, a handle with nmfx_set_ard in
 * force (the relevances are not used in fold-in: nmfx_clear_ard first), no V or no factors (NMFX_E_STATE).
 * W is read from the one buffer that holds it (after nmfx_set_factors; nmfx_get_factors returns it unchanged); a later
 * nmfx_mur_run on the same handle needs nmfx_set_factors first, like a change of solver. */
int nmfx_foldin_run(nmfx_handle_t h, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2,
                    int64_t first, int64_t count);
int nmfx_foldin_finish(nmfx_handle_t h, int distance, int64_t min_iter, double tol1, double tol2, int64_t iters_done);

/* Row-sharded form: phase A = everything up to the rank-local partial sums
 * [W^T V | W^T W | objective], phase B = H update from the (all-reduced) sums.
 * Between the two the caller sum-all-reduces the exchange buffers over ranks
 * (RCCL via torch.distributed, see nmf_amd/dist.py).                          */
int nmfx_mur_phase_a(nmfx_handle_t h, int distance, double lambda_w, int64_t j);
int nmfx_mur_phase_b(nmfx_handle_t h, int distance, double lambda_h,
                     int64_t min_iter, double tol1, double tol2, int64_t j);
/* Phase A in pieces, so that the exchange can overlap with the H-side product (the all-reduce of one column chunk of V runs
 * while the next chunk is computed).  Euclidean loss on the split-bf16 path only: nmfx_mur_chunk_info returns
 * unit = 128 (0: not available for this handle / distance), the padded n and the padded k.  The f32 exchange buffer is
 * [column][factor]: after nmfx_mur_phase_a_cols(h, d, c0, c1) the range xf32[c0 * k_padded, c1 * k_padded) holds this
 * rank's part of (W^T V)[:, c0:c1] and may be reduced; the call whose c1 is the padded n also packs what lies behind the
 * k n part (W^T W, the objective partial), so its range extends to the end of the buffer.  c0, c1: multiples of `unit`,
 * at least 512 columns per call, ascending and without gaps:
 *     nmfx_mur_phase_a_head(j);  for each chunk: nmfx_mur_phase_a_cols(c0, c1), all-reduce of the range (asynchronously);
 *     wait for the reductions;  nmfx_mur_phase_b(j).
 * Results differ from nmfx_mur_phase_a by the summation order of the product's splits only.                            */
int nmfx_mur_chunk_info(nmfx_handle_t h, int distance, int64_t* unit, int64_t* n_padded, int64_t* k_padded);
int nmfx_mur_phase_a_head(nmfx_handle_t h, int distance, double lambda_w, int64_t j);
int nmfx_mur_phase_a_cols(nmfx_handle_t h, int distance, int64_t c0, int64_t c1);
int nmfx_mur_finish_a(nmfx_handle_t h, int distance, int64_t j);
int nmfx_mur_finish_b(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t j);
/* Phase B in two parts, for an exchange by reduce-scatter + all-gather instead of one all-reduce (the sum over the
 * row shards is the one nmf/mur.py:45 `w.T @ x` forms): with `world` ranks, rank r owns the columns [r * cols, (r + 1) * cols) of H,
 *     nmfx_mur_phase_a(j);
 *     reduce-scatter (sum) of xf32[0, world * elems) in place: rank r receives the range [r * elems, (r + 1) * elems);
 *         sum-all-reduce of the rest of the f32 buffer, xf32[world * elems, n_f32)   (W^T W, the objective digits);
 *     nmfx_mur_phase_b_slice(j, r * cols, (r + 1) * cols):   the update of mur.py:45 for those columns, the objective and the stop
 *         rule of iteration j (identical on every rank); the new columns are also left in the rank's range of xf32;
 *     all-gather of the ranges in place;
 *     nmfx_mur_phase_b_rest(r * cols, (r + 1) * cols):       the other ranks' columns into H (and whatever follows the update).
 * nmfx_mur_slice_info returns cols (a multiple of 64) and elems = cols * k_padded, or 0 / 0 where this form is not available:
 * Euclidean loss on the split-bf16 path only (nmfx_set_exchange_rank in force), padded n a multiple of 64 * world.  Every rank ends
 * with bit-identical H: each column is computed by ONE rank and copied.                                                           */
int nmfx_mur_slice_info(nmfx_handle_t h, int distance, int world, int64_t* cols, int64_t* elems);
int nmfx_mur_phase_b_slice(nmfx_handle_t h, int distance, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j,
                           int64_t c0, int64_t c1);
int nmfx_mur_phase_b_rest(nmfx_handle_t h, int distance, int64_t c0, int64_t c1);

/* Exchange buffers: f32 part = [W^T V (kp x n_pad) | W^T W (kp x kp)] (+ KL:
 * column sums of W), f64 part = [objective partial, 4 inner-loop norm sums (sharded AO-ADMM, round by round), 3 spare,
 * 64 x 4 norm sums of the speculative rounds (nmfx_aoadmm_phase_w_fused)].  Sizes in
 * elements.  The caller may supply its own device allocations (e.g. torch
 * tensors, so that torch.distributed can all-reduce them in place).
 * Layout of the f32 part after nmfx_mur_phase_a (kp, n_pad: nmfx_mur_chunk_info), offsets in elements:
 *   [0, kp n_pad)   the product.  Euclidean loss on the split-bf16 path (k padded to 64 / 128, nmfx_get_precision = 1):
 *                   [column][factor], element c * kp + f (nmfx_mur_phase_a_cols, nmfx_mur_phase_b_slice rely on it: a column
 *                   range is contiguous).  Everything else -- KL on that path, the exact-f32 kernels, k > 128 -- :
 *                   [factor][column], element f * n_pad + c.  Padded rows and columns are zero.
 *   kp n_pad        Euclidean: W^T W, [kp][kp].  KL with k <= 128: the kp column sums of W (what follows them up to kp kp is
 *                   unspecified).  KL with k > 128: the column sums lie behind the Gram slot, at kp n_pad + kp kp.
 *   kp n_pad + kp kp + kp    the tail of nmfx_set_exchange_rank: slot r = 4 floats, the 16-bit digits of rank r's objective
 *                   partial, least significant first; phase A writes the slots [0, world) -- its own digits, +0.0 elsewhere.
 * Phase A writes every element phase B reads, and so does nmfx_mur_finish_a for nmfx_mur_finish_b (f64 part [0]): neither buffer
 * needs to be zeroed by the caller, and what a phase does not write (f64 [1, 8) in MUR, tail slots from `world` on, the ranges of
 * other ranks after a reduce-scatter) is never read.  tests/test_gpu_shard_step.py fills all of it with NaN.
 *
 * The phases of the other solvers (declared further down), k <= 128 in either arithmetic mode and composed beyond 128 components.
 * Layout of the f32 part behind every products phase of ADMM, AO-ADMM (both losses) and ANLS (mur_pack_kernel, pack_t_kernel, the
 * generic products): P = [0, kp n_pad + kp kp): the product [factor][column], element f n_pad + c, then the Gram matrix [kp][kp]
 * at kp n_pad; the padded rows and columns of both are exactly zero.  What lies behind P (the column-sum slot of composed MUR-KL,
 * the tail) is neither written nor read by these phases, though the caller's all-reduce of the whole buffer carries it along.
 * "reads" means: after the caller's all-reduce.  "keeps": what has to survive from an EARLIER phase when this one starts;
 * everything else of both buffers may hold anything then (tests/test_gpu_shard_family_step.py makes it NaN before every phase
 * that precedes a collective).
 *   phase                              writes                              reads                               keeps
 *   admm_phase_products(j)             P, f64 [0]                          -                                   composed, j > 0: f64 [0]
 *   admm_phase_update                  composed: f64 [0] of the new pair   P, f64 [0]                          -
 *   aoadmm_phase_h_products(j)         P, f64 [0]                          -                                   composed, j > 0: f64 [0]
 *   aoadmm_phase_h_solve               -                                   P, f64 [0]                          -
 *   aoadmm_phase_w_products            -                                   -                                   -
 *   aoadmm_phase_w_round(r)            f64 [1, 5)                          r > 0: f64 [1, 5) of round r - 1    r > 0: f64 [1, 5)
 *   aoadmm_phase_w_close               composed: f64 [0] of the new pair   f64 [1, 5) of the last round        -
 *   aoadmm_phase_w_fused               f64 [8, 8 + 4 admm_iter)            -                                   -
 *   aoadmm_phase_w_repair              -                                   f64 [8, 8 + 4 admm_iter)            -
 *   aoadmm_kl_phase_h_products(j, r)   r = 0: P, f64 [0]; r > 0: the       -                                   composed, j > 0, r = 0:
 *                                      product (k <= 128: all of P)                                            f64 [0]
 *   aoadmm_kl_phase_h_round(r)         -                                   r = 0: P, f64 [0]; r > 0: the       -
 *                                                                          product part of P
 *   aoadmm_kl_phase_h_close            -                                   -                                   -
 *   aoadmm_kl_phase_w_round(r)         as aoadmm_phase_w_round             as aoadmm_phase_w_round             r > 0: f64 [1, 5)
 *   aoadmm_kl_phase_w_close            composed: f64 [0] of the new pair   f64 [1, 5) of the last round        -
 *   anls_phase_objective               f64 [0]                             -                                   -
 *   anls_phase_w                       P                                   f64 [0]                             f64 [0]
 *   anls_phase_h                       -                                   P                                   -
 *   nmfx_objective_partial             f64 [0]; composed ADMM / AO-ADMM:   -                                   composed ADMM / AO-ADMM:
 *                                      nothing                                                                 f64 [0]
 *   nmfx_mur_finish_b                  -                                   f64 [0]                             -
 * The one value that lives from one outer iteration into the next inside an exchange buffer: beyond 128 components ADMM and
 * AO-ADMM (both losses) close every iteration with the objective partial of the new pair in f64 [0] (phase_update, phase_w_close,
 * and the run entry points alike); the next products phase and nmfx_objective_partial leave it where it is.  Up to 128 components
 * the partials wait in the handle and the products phase / nmfx_objective_partial sum them into f64 [0].
 * No phase reads f64 [5, 8), a table row from admm_iter on, or an element of P it is not listed with.  Behind the inner stop of a
 * KL sub-problem the remaining rounds write and read nothing: their exchanges move whatever the buffers hold.  The W rounds after
 * the stop of the W sub-problem likewise (the all-reduce then multiplies the kept sums by the world's size, which the two ratios
 * of `terminate` do not see).
 * The KL phase entry points are the exact-f32 ones in either arithmetic mode and keep v_aux / dual_v row-major; nmfx_admm_run and
 * nmfx_aoadmm_run in split-bf16 mode keep them tile-major.  A handle changes from the run entry points to the KL phases (or back)
 * only through nmfx_set_factors: otherwise the phases read auxiliaries the run never stored there.                      */
int nmfx_exchange_sizes(nmfx_handle_t h, int64_t* n_f32, int64_t* n_f64);
/* Stream-capture support for the caller-driven loop.  The phase calls only queue launches on the
 * handle's stream, so a caller may capture  phase_a(j=0) . all-reduce . phase_b(j=0) .
 * phase_a(j=1) . all-reduce . phase_b(j=1) . nmfx_shift_iteration_base(+2)  into ONE hipGraph
 * and replay it: the device adds the base to the index each launch carries (objective slot,
 * `i > min_iter` test of nmf/mur.py:131).  Keep the base even (W ping-pong parity), reserve
 * the objective history first (it must not move during replays) and shift the base back to 0
 * before nmfx_mur_finish_* / the run entry points, which take absolute indices. */
int nmfx_reserve_objectives(nmfx_handle_t h, int64_t count);
int nmfx_shift_iteration_base(nmfx_handle_t h, int64_t delta);
/* One collective per outer iteration instead of two (MUR, Euclidean loss, k padded to 64 / 128): with rank / world set, phase A
 * also writes this rank's f64 objective partial into the tail of the f32 exchange buffer -- its four 16-bit digits as exact small
 * floats in the rank's own slot, zeros in the other ranks' slots -- so that the SUM all-reduce of the f32 buffer alone delivers every
 * rank's partial bit for bit; phase B adds them in rank order.  nmfx_exchange_sizes already includes the tail (64 ranks).
 * world = 0 switches back to the separate all-reduce of the f64 buffer.  NMFX_E_STATE when the split-bf16 epilogues are not in use. */
int nmfx_set_exchange_rank(nmfx_handle_t h, int rank, int world);
/* n_f32 / n_f64: the sizes (elements) of the caller's allocations, checked against nmfx_exchange_sizes -- which grew in round 2
 * (f64: 8 -> 8 + 4 * 64 doubles; f32: a tail of 256 floats): a caller that still allocates the old sizes gets NMFX_E_ARG instead of
 * out-of-bounds device writes.  ABI change of version 300 (the two size arguments are new).                                */
int nmfx_set_exchange_buffers(nmfx_handle_t h, void* dev_f32, int64_t n_f32, void* dev_f64, int64_t n_f64);
int nmfx_get_exchange_buffers(nmfx_handle_t h, void** dev_f32, void** dev_f64);

/* ---- the stop rule's referee (r3) ---------------------------------------------------------------------------------------------
 * The objective every iteration records is evaluated in float32 products with float64 sums; near the stop of a long run its
 * iteration-to-iteration jitter (~3e-9 of the objective at 16384 x 8192) is what `new >= old - tol2` (nmf/utils.py:10) sees once
 * tol2 is below ~1e-6 of the objective.  nmfx_objective_f64 evaluates 1/2 ||V - W H||^2 of the CURRENT pair with the product and
 * the sum in float64 (f64 MFMA; ~0.4 ms at 16384 x 8192, k = 64), as the reference's arithmetic would for this iterate.
 * nmfx_set_stop_guard(h, g): the device's rule 2 becomes `new >= old - tol2 - g` -- with g a few times the jitter it fires EARLY, as
 * a candidate; nmfx_resume(h) clears the stop flag so that the caller can walk on one iteration at a time with the f64 objective
 * deciding (nmf_amd._driver.drive, `verify_stop`).  g = 0 (the default) is the plain rule.                                        */
int nmfx_objective_f64(nmfx_handle_t h, double* out);
int nmfx_set_stop_guard(nmfx_handle_t h, double guard);
int nmfx_resume(nmfx_handle_t h);

/* ---- pair mode: two MUR-Euclidean factorizations of the SAME V in one pass over it ------------------------------
 * The reference author's parameter grids (nmf/nmf_old.py:52-66, nmf/nmf.py:38-45) call the solver once per (lambda_w, lambda_h,
 * start); on the GPU two such problems with k <= 64 share the V stream: a handle created with k = 128 holds problem 0 in the
 * factor columns [0, 64) and problem 1 in [64, 128) -- set with ONE nmfx_set_factors call on the stacked, zero-padded m x 128 /
 * 128 x n matrices.  The V-sized products are the k = 128 products; objective, Gram matrices, lambda, stop rule and objective
 * history are per problem (nmf/mur.py:119-136 twice).  A problem whose stop rule fires keeps the iterate the reference returns
 * while the other one continues; the handle's ordinary stop flag is set when both have stopped.  lambda_w / lambda_h: two values
 * each.  Split-bf16 path only (NMFX_E_STATE otherwise); single GPU.                                                            */
int nmfx_mur_pair_run(nmfx_handle_t h, const double* lambda_w, const double* lambda_h, int64_t min_iter, double tol1, double tol2,
                      int64_t first, int64_t count);
int nmfx_mur_pair_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);
int nmfx_pair_get_state(nmfx_handle_t h, int p, int* stop_rule, int64_t* stop_i, int64_t* n_obj);
int nmfx_pair_get_objectives(nmfx_handle_t h, int p, int64_t first, int64_t count, double* out);
int nmfx_pair_get_factors(nmfx_handle_t h, int p, int k_p, double* w, double* hmat);      /* w: m x k_p, hmat: k_p x n */

/* ---- the exchange step behind the C ABI: RCCL over xGMI, one process per GPU -----------------------------------------------
 * north_star: "shard rows of V and W across the 8 GPUs of one node with an RCCL all-reduce over xGMI of the k x k Gram W^T W and
 * the k x n product W^T V each outer iteration" (nmf/mur.py:45 needs w.T @ x and w.T @ w over ALL rows).  RCCL is bound at run
 * time (dlopen librccl.so.1; NMFX_RCCL_LIB overrides the name): NMFX_E_RCCL when it is missing or a call fails.
 *   rank 0:     nmfx_comm_unique_id(id)            -> 128 bytes, handed to the other ranks by the launcher's own means
 *   every rank: nmfx_comm_init_rank(h, id, rank, world)        (h = the handle of this rank's row shard; collective call)
 *               nmfx_comm_negotiate(h)             -> all ranks agree on what fixes the sequence of collectives: the objective
 *                                                     partial inside the f32 buffer (one all-reduce per MUR-eu iteration), the
 *                                                     chunk unit, the arithmetic mode (NMFX_E_STATE if the modes differ)
 *               nmfx_mur_run_sharded(...)          -> `count` outer iterations, each  phase A . all-reduce . phase B  queued on
 *                                                     the handle's stream in ONE call (nmf/mur.py:119-131 for a row shard)
 *               nmfx_mur_finish_sharded(...)       -> objective of the last pair + final stop test (as nmfx_mur_finish)
 * nmfx_comm_all_reduce: in-place SUM over [first, first + count) of the f32 (which = 0) or f64 (which = 1) exchange buffer on the
 * handle's stream -- the exchange of the other solvers' phase entry points (nmfx_aoadmm_phase_*, nmfx_admm_phase_*,
 * nmfx_anls_phase_*).  nmfx_comm_all_min: MIN over the ranks of up to 64 host integers (blocking).
 * nmfx_comm_set_graph(h, 1): nmfx_mur_run_sharded replays pairs of iterations (collectives included) as ONE hipGraph after the
 * first eager pair; a capture that fails leaves the eager loop in charge.  NMFX_DIST_CHUNKS=n: phase A in n column chunks, each
 * chunk's all-reduce on a side stream behind the next chunk's product.                                                       */
int nmfx_comm_unique_id(void* id128);
int nmfx_comm_init_rank(nmfx_handle_t h, const void* id128, int rank, int world);
int nmfx_comm_destroy(nmfx_handle_t h);
int nmfx_comm_info(nmfx_handle_t h, int* rank, int* world, int* merged, int* rccl_version);
int nmfx_comm_negotiate(nmfx_handle_t h);
int nmfx_comm_all_reduce(nmfx_handle_t h, int which, int64_t first, int64_t count);
int nmfx_comm_all_min(nmfx_handle_t h, int64_t* vals, int n);
int nmfx_comm_barrier(nmfx_handle_t h);     /* the handle's queued work is done and every rank has arrived (one-word all-reduce + stream sync) */
int nmfx_comm_set_graph(nmfx_handle_t h, int enable);
/* The exchange inside nmfx_mur_run_sharded: 0 = one sum-all-reduce of the f32 buffer per iteration (default); 1 = reduce-scatter of
 * its W^T V part (+ all-reduce of the k x k Gram matrix and the objective digits, one RCCL group) . nmfx_mur_phase_b_slice .
 * all-gather . nmfx_mur_phase_b_rest -- see nmfx_mur_slice_info.  Iterations the sliced form is not available for take the
 * all-reduce.  The same value on every rank.                                                                                  */
int nmfx_comm_set_exchange(nmfx_handle_t h, int mode);
int nmfx_comm_get_exchange(nmfx_handle_t h, int* mode);
int nmfx_comm_graph_replays(nmfx_handle_t h, int64_t* replays);
int nmfx_mur_run_sharded(nmfx_handle_t h, int distance, double lambda_w, double lambda_h, int64_t min_iter,
                         double tol1, double tol2, int64_t first, int64_t count);
int nmfx_mur_finish_sharded(nmfx_handle_t h, int distance, int64_t min_iter, double tol1, double tol2, int64_t iters_done);

/* ---- initialisation: leading singular triplets of the uploaded V ------------------------
 * Replaces `numpy.linalg.svd(x, full_matrices=False)` in nmf/utils.py:50 for what NNDSVD uses of
 * it (the first `rank` triplets, utils.py:51-82; the construction is invariant under the sign
 * choice of a triplet).  f64 arithmetic on the device: block subspace iteration with
 * Rayleigh-Ritz on `block` columns (0 = max(k + 16, 1.5 k)), stopped when
 * ||V^T u_i - s_i v_i|| <= tol * s_1 for i < k (tol <= 0: 1e-11) or after max_sweeps (<= 0: 4000).
 * u: m x k, s: k, vt: k x n (row-major, host).  sweeps / resid (may be NULL) report the sweeps
 * run and the largest relative residual reached, so the caller can tell a cap from convergence.
 * All k columns of u and rows of vt are orthonormal: a triplet whose Ritz value is numerically zero
 * (V of rank below k) comes back with s_i = 0 and unit vectors orthogonal to the others, and resid
 * covers it too, so a block that lost rank is never reported as converged.  NMFX_E_ARG (with a
 * message): k < 1, k > min(m, n), k > 192, a null u, s or vt; NMFX_E_STATE before nmfx_upload_v. */
int nmfx_topk_svd(nmfx_handle_t h, int k, int block, double tol, int max_sweeps, uint64_t seed,
                  double* u, double* s, double* vt, int* sweeps, double* resid);

/* ---- AO-ADMM (replaces nmf/ao_admm.py:259-301) -------------------------- */
/* One call queues `count` outer iterations: H sub-problem then W sub-problem
 * (admm_ls_update, ao_admm.py:46-68: Gram, rho = trace/k, Cholesky, up to
 * admm_iter rounds of solve / prox / dual update with the `terminate` test of
 * ao_admm.py:33-43 evaluated on the device), objective, convergence check.
 * inner counts per outer iteration are readable with nmfx_get_inner_counts.   */
int nmfx_aoadmm_run(nmfx_handle_t h, int distance, int prox_w, double lambda_w,
                    int prox_h, double lambda_h, int admm_iter,
                    int64_t min_iter, double tol1, double tol2,
                    int64_t first, int64_t count);
/* Row-sharded form (Euclidean loss).  Per outer iteration j the caller runs
 *   phase_h_products . all-reduce(f32, f64) . phase_h_solve . phase_w_products .
 *   { phase_w_round(r) . all-reduce(f64) } for r = 0 .. admm_iter-1 . phase_w_close
 * The H sub-problem (ao_admm.py:263) needs sum_p W_p^T V_p and sum_p W_p^T W_p, after which it
 * is replicated work; the W sub-problem (ao_admm.py:265) is rank-local except that `terminate`
 * (ao_admm.py:33-43) takes norms over ALL rows of W: each round leaves this rank's four sums of
 * squares in the f64 exchange buffer [1..4].  After the last iteration: nmfx_objective_partial .
 * all-reduce(f64) . nmfx_mur_finish_b.                                                      */
int nmfx_aoadmm_phase_h_products(nmfx_handle_t h, int64_t j);
int nmfx_aoadmm_phase_h_solve(nmfx_handle_t h, int prox_h, double lambda_h, int admm_iter,
                              int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_aoadmm_phase_w_products(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_aoadmm_phase_w_round(nmfx_handle_t h, int prox_w, double lambda_w, int round);
int nmfx_aoadmm_phase_w_close(nmfx_handle_t h, int admm_iter, int64_t j);
/* The W sub-problem with ONE exchange: nmfx_aoadmm_phase_w_fused runs all admm_iter (<= 64) rounds speculatively on
 * this rank's rows and leaves its four norm sums of every round in the f64 exchange buffer [8 + 4 round + c];
 * after the caller's all-reduce of those 4 admm_iter numbers nmfx_aoadmm_phase_w_repair derives the round at which
 * `terminate` (ao_admm.py:33-43) fires -- the same on every rank -- reruns that many rounds from the saved start if it
 * is before the last one, records the inner count and leaves the objective partials of the new pair.  Replaces
 * { phase_w_round . all-reduce } x admm_iter . phase_w_close: 3 collectives per outer iteration instead of 2 + admm_iter. */
int nmfx_aoadmm_phase_w_fused(nmfx_handle_t h, int prox_w, double lambda_w, int admm_iter);
int nmfx_aoadmm_phase_w_repair(nmfx_handle_t h, int prox_w, double lambda_w, int admm_iter, int64_t j);

/* Row-sharded AO-ADMM with the KL loss (nmf/ao_admm.py:71-101, 277-283: admm_kl_update for H, then for W on the
 * transposed data).  Its V-sized products sit INSIDE the inner rounds, so the exchange is per round:
 *   for r in range(admm_iter):  nmfx_aoadmm_kl_phase_h_products(j, r); all-reduce(f32 buffer [, f64[0..7] when r == 0]);
 *                               nmfx_aoadmm_kl_phase_h_round(prox_h, lambda_h, r, min_iter, tol1, tol2, j)
 *   nmfx_aoadmm_kl_phase_h_close(admm_iter, min_iter, tol1, tol2, j)
 *   for r in range(admm_iter):  nmfx_aoadmm_kl_phase_w_round(prox_w, lambda_w, r); all-reduce(f64[1..4])
 *   nmfx_aoadmm_kl_phase_w_close(admm_iter, j)
 * The rounds behind the inner stop (`ADMM break`, ao_admm.py:96-98) are no-ops on every rank. */
int nmfx_aoadmm_kl_phase_h_products(nmfx_handle_t h, int64_t j, int round);
int nmfx_aoadmm_kl_phase_h_round(nmfx_handle_t h, int prox_h, double lambda_h, int round, int64_t min_iter, double tol1,
                                 double tol2, int64_t j);
int nmfx_aoadmm_kl_phase_h_close(nmfx_handle_t h, int admm_iter, int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_aoadmm_kl_phase_w_round(nmfx_handle_t h, int prox_w, double lambda_w, int round);
int nmfx_aoadmm_kl_phase_w_close(nmfx_handle_t h, int admm_iter, int64_t j);
/* f64 exchange buffer [0] = this rank's objective partial of the current factor pair.        */
int nmfx_objective_partial(nmfx_handle_t h);
/* Record the objective / convergence test of the last queued iteration.       */
int nmfx_aoadmm_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);
/* Per outer iteration two int32: (H sub-problem, W sub-problem); low 16 bits =
 * inner rounds run, bit 16 = the inner stop test fired ("ADMM break after").  */
int nmfx_get_inner_counts(nmfx_handle_t h, int64_t first, int64_t count, int32_t* out_pairs);

/* ---- ADMM (replaces nmf/admm.py:292-334) -------------------------------- */
/* prox 'l2n' (nmf/admm.py:141-156) solves (1/rho)(lambda T^T T + rho I) X = aux - dual
 * with the k x k second-difference operator T; since rho and lambda are fixed
 * for a run the caller supplies the k x k inverse P (float64, row-major) once:
 * which = 0 for the W regulariser, 1 for H.  The finish call of AO-ADMM
 * (nmfx_aoadmm_finish) is shared by ADMM.                                     */
int nmfx_set_l2n_operator(nmfx_handle_t h, int which, const double* p_inverse);
/* prox 'l1inf' / 'l1inf_transpose' (nmf/admm.py:158-183, :185-210, upper_bound = 1) as one launch on the current
 * ADMM state: side 0: w = prox(w_aux^T, dual_w^T)^T (admm.py:320), side 1: h = prox(h_aux, dual_h) (admm.py:319);
 * update_dual != 0 also does dual += x - x_aux (admm.py:321-322).  nmfx_admm_run calls the same kernels; this entry
 * exists so that the operator can be checked at function level (state through nmfx_set_matrix / nmfx_get_factors).
 * 'l1inf' sorts vectors of n (side 1) or m (side 0) entries in LDS: at most 32768.                                   */
int nmfx_prox_apply(nmfx_handle_t h, int side, int prox, double rho, double lambda, int update_dual);
int nmfx_admm_run(nmfx_handle_t h, int distance, double rho, int prox_w, double lambda_w,
                  int prox_h, double lambda_h, int64_t min_iter, double tol1,
                  double tol2, int64_t first, int64_t count);
/* Row-sharded form.  Per outer iteration j:  phase_products . all-reduce(f32, f64) . phase_update
 * phase_products leaves this rank's [w_aux^T V | w_aux^T w_aux] (KL loss: w_aux^T (v_aux + dual_v)) and the objective
 * partial of the current pair in the exchange buffers (j = 0: also the start state of admm.py:27-28, 289);
 * phase_update records obj[j] / evaluates the stop rule, solves h_aux from the all-reduced sums (replicated work,
 * admm.py:295), solves this rank's rows of w_aux (admm.py:297), applies both prox operators and dual updates
 * (admm.py:319-322).  ADMM has no inner loop: this is the only exchange.  After the last iteration:
 * nmfx_objective_partial . all-reduce(f64) . nmfx_mur_finish_b.  The row-coupled prox 'l1inf' on the W side and
 * 'l1inf_transpose' on the W side (column 1 of dual_w^T = global row 1) are not available sharded.                   */
int nmfx_admm_phase_products(nmfx_handle_t h, int distance, double rho, int prox_w, int prox_h, int64_t j);
int nmfx_admm_phase_update(nmfx_handle_t h, int distance, double rho, int prox_w, double lambda_w,
                           int prox_h, double lambda_h, int64_t min_iter, double tol1, double tol2, int64_t j);

/* ---- ANLS (replaces nmf/anls.py:111-122) -------------------------------- */
/* distance_type of ANLS (nmf/anls.py:108,118): NMFX_EU (default) or NMFX_KL.  It only selects the objective that is
 * recorded and tested by the stop rule; the iterates are the least-squares ones either way, as in the reference.   */
int nmfx_anls_set_distance(nmfx_handle_t h, int distance);
int nmfx_anls_run(nmfx_handle_t h, double lambda_w, double lambda_h,
                  int64_t min_iter, double tol1, double tol2,
                  int64_t first, int64_t count);
/* Row-sharded form.  Per outer iteration j:
 *   phase_objective . all-reduce(f64) . phase_w . all-reduce(f32) . phase_h
 * phase_w records obj[j] / evaluates the stop rule, solves the rank's rows of W (anls.py:18-31)
 * and leaves [W^T V | W^T W] partials in the exchange buffer; phase_h solves all columns of H
 * (replicated, anls.py:34-47).  After the last iteration: nmfx_objective_partial .
 * all-reduce(f64) . nmfx_mur_finish_b.                                                      */
int nmfx_anls_phase_objective(nmfx_handle_t h, int64_t j);
int nmfx_anls_phase_w(nmfx_handle_t h, double lambda_w, int64_t min_iter, double tol1, double tol2, int64_t j);
int nmfx_anls_phase_h(nmfx_handle_t h, double lambda_h, int64_t j);

/* ---- HALS (hierarchical alternating least squares, Cichocki & Phan 2009) -- */
/* The iteration of nmfx_anls_run with each exact NNLS solve replaced by `sweeps` (1 .. 16) projected Gauss-Seidel sweeps over
 * the k components, started from the current row of W / column of H:
 *     for j = 0 .. k-1:  if G[j][j] > 0:  x[j] = max(0, x[j] + (r[j] - sum_l G[j][l] x[l]) / G[j][j])
 * on the same G = F^T F + 2 lambda I and r = F^T b.  Objective, stop rule and history as nmfx_anls_run; nmfx_anls_set_distance
 * selects the recorded objective and nmfx_aoadmm_finish closes the run.  Dense handles without weights, k <= 128
 * (NMFX_E_ARG otherwise, and for sweeps outside 1 .. 16, a negative lambda or a negative range).                        */
int nmfx_hals_run(nmfx_handle_t h, double lambda_w, double lambda_h, int sweeps,
                  int64_t min_iter, double tol1, double tol2,
                  int64_t first, int64_t count);

/* ---- HALS beyond 128 components (version 396) ------------------------------------------------------------------------------
 * The iteration of nmfx_hals_run on a dense handle without weights and 128 < k <= 1024, on the products of nmfx_anls_run beyond
 * 128 components: both Gram matrices in exact f32, the two V-sized products in the handle's arithmetic mode, then `sweeps`
 * sweeps of the rule above per row of W / column of H by a kernel that streams G through LDS in row tiles.
 * Update order, the exact-zero clamp, a component with G_jj = 0 keeping its value and the zero padding are those of
 * nmfx_hals_run; no atomics, two runs give the same bits.  Records, stop rule, nmfx_anls_set_distance and the closing
 * nmfx_aoadmm_finish as nmfx_hals_run; the family in the entry guard is HALS's, so nmfx_anls_run does not continue its run
 * without nmfx_set_factors (NMFX_E_STATE).  NMFX_E_ARG, nothing launched: a sparse handle, a handle with weights, k <= 128
 * (nmfx_hals_run serves those), k > 1024, and the argument rules of nmfx_hals_run.                                            */
int nmfx_hals_wide_run(nmfx_handle_t h, double lambda_w, double lambda_h, int sweeps,
                       int64_t min_iter, double tol1, double tol2,
                       int64_t first, int64_t count);

/* ---- HALS on sparse handles (version 391) ----------------------------------------------------------------------------------
 * The outer iteration of nmfx_hals_run on an unmasked nmfx_create_csr handle with k <= 128: the W half-step, then the H
 * half-step, each `sweeps` sweeps per row of W / column of H on G = the other factor's Gram + 2 lambda I and r summed from
 * the non-zeros; V is never densified.  One launch per half-step gathers r and runs the sweep (plus one for the rows longer
 * than a piece); the H half-step also sums <h_c, r_c> in f64, so the Euclidean objective of the new pair,
 *     1/2 [ ||X||^2 - 2 Sum_c <h_c, W^T x_c> + <W^T W, H H^T> ]      (everything in f64 over the f32 factors),
 * costs no third pass over the non-zeros.  nmfx_hals_sparse_run records obj[0] when first == 0 and obj[j + 1] at the end of
 * iteration j, where the stop rule for loop index j is evaluated; once it has fired the later iterations of the call do
 * nothing and the factors are the pair the last recorded objective belongs to.  nmfx_hals_sparse_finish records
 * obj[iters_done] only where it does not exist yet.  Two runs give the same bits.
 * NMFX_E_ARG with a message, nothing launched: a dense handle, a masked handle, k padded to 256, sweeps outside 1 .. 16, a
 * negative lambda or range.  The run is of the HALS family: on a sparse handle neither nmfx_mur_run nor nmfx_hals_sparse_run
 * continues the other's run without nmfx_set_factors (NMFX_E_STATE).  nmfx_hals_run itself stays dense-only.             */
int nmfx_hals_sparse_run(nmfx_handle_t h, double lambda_w, double lambda_h, int sweeps,
                         int64_t min_iter, double tol1, double tol2,
                         int64_t first, int64_t count);
int nmfx_hals_sparse_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);

/* ---- HALS on sparse handles with 129 .. 256 components (version 397) -------------------------------------------------------
 * The outer iteration of nmfx_hals_sparse_run on an unmasked nmfx_create_csr handle with 128 < k <= 256 (kp = 256), where the
 * Gram matrix no longer fits in LDS beside the gather: each half-step is a gather launch that leaves r of every row of W /
 * column of H in a buffer (plus one launch for the rows longer than a piece) and then the tiled sweep of nmfx_hals_wide_run on
 * G = the other factor's Gram + 2 lambda I.  The H half-step sums r in f64, keeps it in f64 and rounds it for
 * the sweep only; a reduction sums <h_c, r_c> in f64 behind the sweep, so the objective costs no third pass over the non-zeros.
 * Update order, the exact-zero clamp, a component with G_jj = 0 keeping its value and the zero padding are those of
 * nmfx_hals_sparse_run; records, the stop flag, obj[0] when first == 0 and nmfx_hals_sparse_wide_finish as the
 * nmfx_hals_sparse_* pair.  No atomics: two runs give the same bits.  HALS family (NMFX_E_STATE when nmfx_mur_run continues
 * its run without nmfx_set_factors).  NMFX_E_ARG with a message, nothing launched: a dense handle, a masked handle, k <= 128
 * (nmfx_hals_sparse_run serves those), sweeps outside 1 .. 16, a negative lambda or range.                                  */
int nmfx_hals_sparse_wide_run(nmfx_handle_t h, double lambda_w, double lambda_h, int sweeps,
                              int64_t min_iter, double tol1, double tol2,
                              int64_t first, int64_t count);
int nmfx_hals_sparse_wide_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);

/* ---- HALS on masked handles (version 392) ----------------------------------------------------------------------------------
 * The same outer iteration on a masked handle (nmfx_set_masked) with k <= 64: only the stored entries are part of the fit,
 * so every row of W / column of H is swept on a system of its own,
 *     G = Sum_{e in Omega} f_e f_e^T + 2 lambda I,    r = Sum_{e in Omega} v_e f_e,
 * Omega the observed set of that row or column and f_e the gathered row of the other factor (for the H half-step the W just
 * updated).  A stored zero is data: it adds to G and not to r.  A component with G_jj = 0 keeps its value (with lambda = 0:
 * every component of a row with no observed entry, and a dead component).  One launch per half-step forms G and r on the f32
 * MFMA pipe and sweeps (plus one for the rows longer than a piece); a third pass sums the recorded objective
 * 1/2 Sum_Omega (v - wh)^2 per entry in f64.  Records, stop rule, the flag and nmfx_hals_masked_finish as the
 * nmfx_hals_sparse_* pair.  Two runs give the same bits.
 * NMFX_E_ARG with a message, nothing launched: a dense handle, an unmasked handle ("masked handle"), k padded beyond 64,
 * sweeps outside 1 .. 16, a negative lambda or range.  HALS family: NMFX_E_STATE when continuing another solver's run
 * without nmfx_set_factors.  nmfx_hals_sparse_* and nmfx_hals_run go on refusing masked handles.                          */
int nmfx_hals_masked_run(nmfx_handle_t h, double lambda_w, double lambda_h, int sweeps,
                         int64_t min_iter, double tol1, double tol2,
                         int64_t first, int64_t count);
int nmfx_hals_masked_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);

/* ---- HALS fold-in (version 393) -------------------------------------------------------------------------------------------
 * Least-squares H for the handle's V against a fixed W: the handle is an nmfx_create_csr handle of the NEW data with the
 * factors set (nmfx_set_factors(w, h0)), unmasked with k <= 128 or masked (nmfx_set_masked) with k <= 64.  W is never touched.
 * With W fixed a column's system depends on V and W only -- G = W^T W + 2 lambda_h I and r_c = W^T v_c, or on a masked handle
 * the column's own G_c = Sum_Omega w_e w_e^T + 2 lambda_h I and r_c = Sum_Omega v_e w_e -- so it is formed once (one gather of
 * V) and the projected Gauss-Seidel sweeps of the HALS H half-step run on it in place, column by column, from h0[:, c]:
 * after sweep s, d_s is the largest step |delta_j| of that sweep and xmax_s the largest component after it; the column stops
 * after the first s with d_s <= tol xmax_s (d_s = 0 included), or after max_sweeps.  The kept residual r - G x is formed anew
 * before the sweeps 17, 33, ...  With tol = 0 and max_sweeps = s <= 16 the result is, bit for bit, the H half-step of
 * nmfx_hals_sparse_run / nmfx_hals_masked_run with sweeps = s from the same (W, H).  Padded components are exact zeros, a
 * component with G_jj = 0 keeps its value, no atomics: two runs give the same bits.
 * nmfx_hals_foldin_run records obj[0] of the start and obj[1] of the result (nmfx_get_objectives; the objective its family
 * records, at lambda_w = 0), and the stop rule of the outer loop never fires.  HALS family (NMFX_E_STATE when continuing
 * another solver's run without nmfx_set_factors); the H-side statistics of an unmasked handle are current again on return.
 * NMFX_E_ARG with a message, nothing launched: a dense handle, a masked handle with k padded beyond 64, k padded beyond 128, a
 * NaN or negative tol or tol >= 1, max_sweeps outside 1 .. 10000, a lambda_h that is not >= 0.
 * nmfx_hals_foldin_get_sweeps: out[n] = the sweeps each column took; NMFX_E_STATE if no solve has run since the factors were set. */
int nmfx_hals_foldin_run(nmfx_handle_t h, double lambda_h, double tol, int max_sweeps);
int nmfx_hals_foldin_get_sweeps(nmfx_handle_t h, int32_t* out /* n */);

/* ---- dense HALS fold-in (version 394) ------------------------------------------------------------------------------------
 * The same solve for DENSE new data: the handle is an nmfx_create handle of the new data without weights, k <= 128, with the
 * factors set (nmfx_set_factors(w, h0)).  W is never touched.  Every column shares G = W^T W + 2 lambda_h I and r_c is column c
 * of W^T V: the products of the H half-step of nmfx_hals_run, formed ONCE in the handle's arithmetic mode (one pass over V);
 * then every column is swept in place from h0[:, c] under the stop rule above (d_s <= tol xmax_s, or max_sweeps; the kept
 * residual formed anew before the sweeps 17, 33, ...) -- k x n work that never reads V again.  With tol = 0 and
 * max_sweeps = s <= 16 the result is, bit for bit, the H half-step of nmfx_hals_run with sweeps = s from the same (W, H).
 * Padded components are exact zeros, a component with G_jj = 0 keeps its value, no atomics: two runs give the same bits.
 * nmfx_hals_foldin_dense_run records obj[0] of the start and obj[1] of the result (nmfx_get_objectives), each 1/2 ||V - W H||^2
 * with product and sum in f64: the quantity nmfx_objective_f64 returns, bit for bit.  nmfx_get_state reports 2 objectives and the
 * stop rule of the outer loop never fires.  HALS family (NMFX_E_STATE when continuing another solver's run without
 * nmfx_set_factors).  On a handle whose stop rule has already fired (an nmfx_hals_run that stopped, no nmfx_set_factors since)
 * the call launches but moves nothing, as every solver does there: the iterate stays, nothing is recorded, and the counts are
 * not those of a solve.
 * NMFX_E_ARG with a message, nothing launched: a sparse handle, a handle with per-entry weights, k padded beyond 128, a NaN or
 * negative tol or tol >= 1, max_sweeps outside 1 .. 10000, a lambda_h that is not >= 0.
 * nmfx_hals_foldin_dense_get_sweeps: out[n] = the sweeps each column took; NMFX_E_STATE if no dense fold-in has run since the
 * factors were set.  nmfx_hals_foldin_run / nmfx_hals_foldin_get_sweeps are as they were: sparse handles only. */
int nmfx_hals_foldin_dense_run(nmfx_handle_t h, double lambda_h, double tol, int max_sweeps);
int nmfx_hals_foldin_dense_get_sweeps(nmfx_handle_t h, int32_t* out /* n */);

/* ---- MUR fold-in on sparse and masked handles (version 395) ---------------------------------------------------------------
 * H for the handle's V against a fixed W under the loss of sparse / masked MUR: the handle is an nmfx_create_csr handle of the
 * NEW data, masked (nmfx_set_masked) or not, with the factors set (nmfx_set_factors(w, h0)), any k the handle takes (k <= 256).
 * W is never written; H is updated in place.  With W fixed the columns of H are independent problems: column c repeats the H
 * half-step of nmfx_mur_run on this handle -- entries e = (i_e, x_e) the column's non-zeros, or its observed cells on a masked
 * handle, w_e row i_e of W, q_e = <w_e, h>, lambda = lambda_h --
 *     unmasked NMFX_EU   h' = h a / (h G + lambda h + 1e-9)              a = Sum x_e w_e,  G = W^T W
 *     unmasked NMFX_KL   h' = 2 h a / (s + sqrt(s^2 + 4 lambda h a))     a = Sum x_e / (q_e + 1e-9) w_e,  s = colsum W
 *     masked NMFX_EU     h' = h a / (d + lambda h + 1e-9)                a = Sum x_e w_e,  d = Sum q_e w_e
 *     masked NMFX_KL     h' = 2 h a / (d + sqrt(d^2 + 4 lambda h a))     a as unmasked,  d = Sum w_e;  d = 0 -> 0
 *     masked NMFX_IS     h' = h sqrt(a / (d + lambda))                   a = Sum x_e / (q_e + 1e-9)^2 w_e,  d = Sum w_e / (q_e + 1e-9);  d + lambda = 0 -> 0
 * in one launch, the iterate in registers: after step t, delta_t = max_j |h'_j - h_j| and xmax_t = max_j h'_j; the column stops
 * after the first t with delta_t <= tol xmax_t (delta_t = 0 included), or after max_iter.  One step of a column of at most 256
 * entries is the H half-step bit for bit.  Padded components are exact zeros, no atomics: two runs give the same bits.
 * nmfx_sparse_foldin_run records obj[0] of the start and obj[1] of the result (nmfx_get_objectives), as nmfx_mur_run records the
 * objective of that loss on this handle at lambda_w = 0; the stop rule of the outer loop never fires.  MUR family (NMFX_E_STATE when
 * continuing another solver's run without nmfx_set_factors, and after nmfx_mur_run has iterated on the handle since the factors
 * were set); the H-side statistics of an unmasked handle are current again on return.
 * NMFX_E_ARG with a message, nothing launched: a dense handle (nmfx_foldin_run takes those, and keeps refusing sparse ones),
 * NMFX_IS on an unmasked handle, NMFX_BETA or an unknown distance, a NaN or negative tol or tol >= 1, max_iter outside 1 .. 10000,
 * a lambda_h that is not >= 0.
 * nmfx_sparse_foldin_get_iters: out[n] = the steps each column took; NMFX_E_STATE unless nmfx_sparse_foldin_run has run since
 * the factors were set (nmfx_hals_foldin_get_sweeps keeps a flag of its own: neither getter answers for the other's run). */
int nmfx_sparse_foldin_run(nmfx_handle_t h, int distance, double lambda_h, double tol, int max_iter);
int nmfx_sparse_foldin_get_iters(nmfx_handle_t h, int32_t* out /* n */);

/* ---- stacked HALS (version 390)------------------------------------------------------------------------------------------
 * MANY least-squares factorizations of the same V in one pass over it: P problems sit side by side in the factor columns,
 * W = [W_0 | W_1 | ...], H = [H_0; H_1; ...].  The V-sized products V H^T and W^T V of the stacked factors are the P problems'
 * products, and with the Gram entries between different problems masked the Gauss-Seidel sweep over all components is P
 * independent sweeps: problem p's iterates are those of nmfx_hals_run on a handle of its own.  Dense handles without weights,
 * k <= 128 (NMFX_E_ARG otherwise, nothing launched).  A family of its own: hals, anls, mur and the stack do not continue
 * each other without nmfx_set_factors.
 *
 * nmfx_hals_stack_set: problem p owns the components [o_p, o_p + k_p), o_p = sum_{q < p} k_q; every k_p >= 1 and their sum
 * <= the handle's k (NMFX_E_ARG).  Components past the last problem belong to none: set them to zero, they stay zero.
 * nprob = 0 clears the stack.  Call it after nmfx_set_factors and before the run (NMFX_E_STATE once a solver has run on the
 * factors); the partition survives nmfx_set_factors, which starts every problem's stop state and history anew.
 *
 * nmfx_hals_stack_terms: out[nprob][2] = <V, W_p H_p> and ||W_p H_p||^2 of the current factors (the least-squares scale of
 * a start is their quotient).
 *
 * nmfx_hals_stack_run / _finish: as nmfx_hals_run / nmfx_aoadmm_finish, with lambda_w[nprob], lambda_h[nprob].  The objective
 * of problem p after j iterations, recorded at obj_p[j], is
 *     1/2 ||V||^2 - sum_i sum_{c in p} W_ic (V H^T)_ic + 1/2 <(W^T W)_pp, (H H^T)_pp>
 * with ||V||^2, both Gram blocks and both sums in f64 over the f32 factor values and the f32 product V H^T.  Each problem has
 * its own stop rule (that of nmfx_hals_run, on obj_p) and keeps its iterate from its stop on while the others go on; no f64
 * referee stands behind this objective (nmfx_set_stop_guard does not apply).  nmfx_get_state reports a stop once ALL problems
 * have stopped.
 *
 * nmfx_hals_stack_get_state / _get_objectives / _get_factors: problem p's stop rule, stop index, number of recorded objectives;
 * obj_p[first .. first + count); w (m x k_p) and hmat (k_p x n).                                                             */
int nmfx_hals_stack_set(nmfx_handle_t h, int nprob, const int* k_p);
int nmfx_hals_stack_terms(nmfx_handle_t h, double* out);
int nmfx_hals_stack_run(nmfx_handle_t h, const double* lambda_w, const double* lambda_h, int sweeps,
                        int64_t min_iter, double tol1, double tol2, int64_t first, int64_t count);
int nmfx_hals_stack_finish(nmfx_handle_t h, int64_t min_iter, double tol1, double tol2, int64_t iters_done);
int nmfx_hals_stack_get_state(nmfx_handle_t h, int p, int* stop_rule, int64_t* stop_i, int64_t* n_obj);
int nmfx_hals_stack_get_objectives(nmfx_handle_t h, int p, int64_t first, int64_t count, double* out);
int nmfx_hals_stack_get_factors(nmfx_handle_t h, int p, double* w, double* hmat);

/* ---- measurement -------------------------------------------------------- */
/* Accumulated device time (HIP events on the handle's stream) and launch count
 * of a named kernel since the last reset; names: "wphase" "hphase" ...        */
int nmfx_profile_enable(nmfx_handle_t h, int on);
int nmfx_profile_get(nmfx_handle_t h, const char* name, double* total_ms, int64_t* launches);
int nmfx_profile_reset(nmfx_handle_t h);
/* Mean duration of ONE product kernel of MUR -- which = "wphase" (V H^T + objective, nmf/mur.py:29 + utils.py:29)
 * or "hphase" (W^T V, nmf/mur.py:45), distance NMFX_EU / NMFX_KL -- over `reps` back-to-back launches on the
 * handle's stream between one pair of HIP events (two untimed launches first).  The launches recompute the
 * products of the current factors; no factor is modified.  This is the live per-launch time `bench.py` divides
 * the algorithmic bytes by: a HIP event in front of EVERY launch (nmfx_profile_enable) puts a command-processor
 * barrier there, which the loop of a real factorisation does not have.                                        */
int nmfx_profile_repeat(nmfx_handle_t h, const char* which, int distance, int reps, double* ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* NMFX_H */
