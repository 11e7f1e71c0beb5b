/*
 * autogp_hip.h — C ABI of the MI355X-native GP marginal-likelihood engine.
 *
 * Drop-in boundary for the hot path of probsys/AutoGP.jl (reference paths are
 * relative to the upstream repo):
 *
 *   value path       src/Model.jl:134-136   noise+JITTER, GP.compute_cov_matrix_vectorized,
 *                                           xs ~ mvnormal(zeros(n), K)  (Cholesky/logdet/solve
 *                                           happen inside Gen/Distributions/PDMats -> dpotrf)
 *   matrix assembly  src/GP.jl:666-668      eval_cov(node, ts) + noise*I
 *   predictive path  src/GP.jl:731-758      Distributions.MvNormal(node, noise, ts, xs, ts_pred;
 *                                           noise_pred, mean), called from
 *                                           src/inference_utils.jl:174-196
 *
 * The reference has no FFI for this path (it is pure Julia); these entry points are what a
 * `ccall` shim replacing those two call sites binds.  Plain pointers and
 * sizes only; all arrays are Julia-native: column-major, Float64 / Int32 / UInt8.
 *
 * Kernel program encoding (one per particle): POSTFIX over the kernel tree, i.e. the order of
 * `unroll(node)` (src/GP.jl:112-113: left, right, node).  Opcodes are the GPConfig node codes
 * (src/GP.jl:1101-1108) plus 0 for WhiteNoise:
 *     0 WhiteNoise{value}                         (src/GP.jl:131-140)
 *     1 Constant{value}                           (src/GP.jl:157-166)
 *     2 Linear{intercept,bias,amplitude}          (src/GP.jl:185-203)
 *     3 SquaredExponential{lengthscale,amplitude} (src/GP.jl:228-245)
 *     4 GammaExponential{lengthscale,gamma,amplitude} (src/GP.jl:269-289)
 *     5 Periodic{lengthscale,period,amplitude}    (src/GP.jl:315-336)
 *     6 Plus   7 Times                            (src/GP.jl:358-377, 404-423)
 *     8 ChangePoint{location,scale}               (src/GP.jl:466-503)
 * Parameters are the TRANSFORMED values in struct-field order, concatenated in program order
 * (ChangePoint contributes location, scale at its own position).
 *
 * Error convention: every call returns 0 on success, <0 on API/HIP failure (text via
 * agp_last_error).  Numerical failure is per particle, LAPACK dpotrf style:
 * out_info[p] = k > 0  => leading minor k is not positive definite, out_logpdf[p] = NaN
 * (the Julia shim rethrows LinearAlgebra.PosDefException(k), reproducing the reference's
 * abort-on-non-PD behaviour).  n = 0 => logpdf = 0, info = 0
 * (src/inference_smc_anneal_data.jl:185-187 initialises the particle filter on 0 points).
 *
 * Threading: agp_logpdf / agp_logpdf_batch / agp_predict_batch / agp_cov_matrix are safe for
 * concurrent callers on one context (one call per Julia `Threads.@threads` iteration,
 * src/inference_smc_anneal_data.jl:133,240); each call takes a private stream+workspace slot.
 * agp_init / agp_destroy / agp_set_data are called from one thread between parallel regions.
 *
 * Ownership: the caller owns every host buffer; the library copies what it needs before
 * returning and owns all device memory.
 */
#ifndef AUTOGP_HIP_H
#define AUTOGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct agp_ctx agp_ctx;

#define AGP_OK               0
#define AGP_ERR_ARG         -1
#define AGP_ERR_HIP         -2
#define AGP_ERR_PROGRAM     -3   /* malformed postfix program / unsupported tree shape */
#define AGP_ERR_NODATA      -4
#define AGP_ERR_COMM        -5   /* RCCL unavailable / collective failed */
#define AGP_ERR_HOST        -6   /* host allocation failure or any other C++ exception, stopped at the C boundary */

#define AGP_MAX_OPS        255   /* nodes per kernel tree (depth-6 full tree = 63) */

/* One context per GPU.  Multi-GPU deployments: one process per GPU (agp_init + agp_comm_init_rank), or one host
 * process driving every GPU of the node (agp_init_multi) — see the multi-GPU section below. */
int  agp_init(agp_ctx** out, int device_id);
void agp_destroy(agp_ctx* ctx);
const char* agp_last_error(agp_ctx* ctx);
const char* agp_version(void);

/* Upload the (already rescaled) observations once; later calls use the prefix n <= n_max —
 * the data-annealing schedule evaluates on ts[1:step] (src/inference_smc_anneal_data.jl:206-217). */
int agp_set_data(agp_ctx* ctx, const double* ts, const double* xs, int64_t n_max);

/* Single particle — what Gen's interpreter calls at src/Model.jl:135-136.  Re-entrant.  Concurrent
 * callers (one per Julia thread, src/inference_smc_anneal_data.jl:133-135) are coalesced inside the
 * library into one batched sweep: the first arrival gathers the others for at most the coalescing window
 * (default 2000 us, and never more than a quarter of the previous sweep's duration; env AGP_COALESCE_US,
 * agp_set_coalesce_window; 0 disables).  A lone caller never waits, and the gathering stops as soon as every thread that has ever
 * called is queued.  While sweeps are short (< 1.5 ms: the reference's tutorial sizes) up to AGP_SPIN (default 8; 0 = never) waiting
 * callers spin on their result for about one sweep before they sleep — a futex wake-up costs ~50 us, a sweep of eight 144-point
 * particles ~200. */
int agp_logpdf(agp_ctx* ctx, int64_t n,
               const uint8_t* ops, int32_t n_ops, const double* prm, int32_t n_prm,
               double noise, double* out_logpdf, int32_t* out_info);

/* P particles in one sweep.  op_off / prm_off have P+1 entries (CSR offsets into ops / prm).
 * noise[p] is the value after `transform_param(:noise, z) + JITTER` (src/Model.jl:134). */
int agp_logpdf_batch(agp_ctx* ctx, int64_t n, int32_t P,
                     const int32_t* op_off, const uint8_t* ops,
                     const int32_t* prm_off, const double* prm,
                     const double* noise,
                     double* out_logpdf /* P */, int32_t* out_info /* P */);

/* Many SHORT series scored in one call: one workgroup per particle, covariance, Cholesky factor, forward solve and value all in LDS
 * (a 144-point series is two mostly padded 128 x 128 tile rows on the tiled path; here it is 45 blocks of 16 x 16 in one CU's LDS).
 * S independent series, concatenated: series s is ts[pt_off[s] .. pt_off[s+1]), xs likewise (already rescaled).
 * P particles; particle p scores series series[p]:
 *   out_logpdf[p] = log N(xs_s; 0, K_p(ts_s) + noise[p] I).
 * Same program encoding, noise meaning and per-particle info conventions as agp_logpdf_batch: out_info[p] = k > 0 is the 1-based index,
 * within the particle's OWN series, of the first non-positive pivot, and out_logpdf[p] is then NaN; a series of length 0 gives
 * logpdf 0 and info 0.  P == 0 is AGP_OK and touches nothing.
 * AGP_SERIES_MAX_N: the LDS budget of one workgroup (160 KiB) holds ceil(n/16) (ceil(n/16) + 1) / 2 blocks of 2 KiB — 132 KiB at 176
 * points — beside ~7 KiB of vectors, tables and program, which leaves room for 10 ChangePoint tables of 2 KiB at the cap.
 * The WHOLE call is rejected — there is no fall-back through the resident-series path — with
 *   AGP_ERR_ARG (the message names the series or particle): null pointers, negative S or P, pt_off[0] != 0, a decreasing pt_off,
 *     series[p] outside [0, S), a series longer than AGP_SERIES_MAX_N, malformed op_off / prm_off;
 *   AGP_ERR_PROGRAM (names the particle): a malformed program, as agp_logpdf_batch reports it, or one whose per-point tables
 *     (ChangePoint nodes) do not fit the LDS budget at that series' length.
 * Stateless: needs no agp_set_data; reads and changes nothing the context holds for its resident series — the series itself, the
 * factor store and its statistics, lag / lattice / compact tables, the coalescer, dedup and mixture counters.  (With profiling on,
 * agp_get_timing's out[0] = out[2] = the call's kernel time, the rest 0.)  Copies of a particle are NOT deduplicated.
 * As re-entrant as agp_logpdf_batch (a private stream and workspace slot per call).  A particle's result bits depend only on its own
 * series, program, parameters and noise — not on what else is in the call, its order, or how the call is split into launches. */
#define AGP_SERIES_MAX_N 176
int agp_logpdf_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                            int32_t P, const int32_t* series /* P */,
                            const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                            const double* noise, double* out_logpdf /* P */, int32_t* out_info /* P */);

/* agp_logpdf_series_batch for series of up to AGP_LONG_SERIES_MAX_N = 512 points (the reference's 442-point data set beside its 135-
 * and 143-point ones in ONE call).  Every convention is agp_logpdf_series_batch's: program encoding, noise meaning, out_info (the
 * 1-based first non-positive pivot within the particle's own series, out_logpdf[p] NaN then), an empty series gives logpdf 0 and
 * info 0, P == 0 is AGP_OK and touches nothing; stateless (no agp_set_data; the resident series, the factor store, the tables and
 * every counter are neither read nor changed), re-entrant (a private stream and workspace slot per call), copies of a particle are
 * not deduplicated, and with profiling on agp_get_timing's out[0] = out[2] = the call's kernel time.
 * Routing: a series of at most AGP_SERIES_MAX_N points runs in agp_logpdf_series_batch's kernel and its result is bit-identical to
 * that entry's.  A longer series runs in k_long_series_logpdf: one workgroup per particle, the Cholesky factor in a per-workgroup
 * HBM workspace (packed 16 x 16 blocks, 1.03 MiB at 512 points), left-looking by block columns on v_mfma_f64_16x16x4, the forward
 * solve carried along.  flags & AGP_LONG_SERIES_ALL: every non-empty series takes that kernel, whatever its length (one arithmetic
 * for the whole family).
 * The workspace comes from the call's slot; one launch takes at most min(agp_set_workspace_limit's value, 1 GiB) of it (the default
 * limit likewise capped at 1 GiB: about 990 particles of 512 points) and a call with more long particles is split into several
 * launches on its stream.  A particle's result bits depend only on its own series, program, parameters, noise and the flag — not on
 * what else is in the call, its order, or the split.
 * The WHOLE call is rejected, outputs untouched, with
 *   AGP_ERR_ARG (the message names the series or particle): everything agp_logpdf_series_batch lists, the cap now
 *     AGP_LONG_SERIES_MAX_N (the message gives the series, its length and that name); flag bits other than AGP_LONG_SERIES_ALL;
 *   AGP_ERR_PROGRAM (names the particle): a malformed program, or one whose per-point tables do not fit the kernel's LDS at that
 *     series' length.  The long kernel keeps 4 KiB per ChangePoint node (a 512-entry table) beside 21 KiB of vectors, tables and one
 *     diagonal block and the program: at 512 points a chain of 10 ChangePoint nodes takes 61 KiB (two workgroups share a CU), 34
 *     nodes beside a small program are the most 160 KiB hold, 40 are refused.
 * The forecast and its band above AGP_SERIES_MAX_N points: agp_predict_long_series_batch, agp_predict_quantile_long_series_batch;
 * the held-out scores: agp_predict_logpdf_long_series_batch.
 * Not here: gradient, sampling, decomposition and HMC twins above AGP_SERIES_MAX_N points; series beyond
 * AGP_LONG_SERIES_MAX_N; deduplication inside a call. */
#define AGP_LONG_SERIES_MAX_N 512
#define AGP_LONG_SERIES_ALL 1   /* flags: every non-empty series takes the long kernel */
int agp_logpdf_long_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                 int32_t P, const int32_t* series /* P */,
                                 const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                 const double* noise, int32_t flags, double* out_logpdf /* P */, int32_t* out_info /* P */);

/* Value AND gradient of many short series in one call: agp_logpdf_series_batch's twin for Gen.choice_gradients / Gen.map_optimize of
 * callers that hold one model per short series.  One workgroup per particle forms, behind the value and in the same LDS, L^-T in place
 * of L, alpha = K^-1 x, and contracts G = 1/2 (alpha alpha' - K^-1) with dK / d theta block by block; K^-1 is never stored and nothing
 * but the outputs leaves the compute unit.
 * Series, program, noise and info conventions are exactly those of agp_logpdf_series_batch; out_logpdf[p] is bit-identical to what
 * that entry returns for the same particle.  out_grad has agp_logpdf_grad_batch's layout (the caller's parameter order, block p at
 * prm_off[p]; ChangePoint contributes location and scale); out_grad_noise[p] = d logpdf / d noise = tr G.
 * A series of length 0 gives logpdf 0, a zero gradient block, grad_noise 0 and info 0.  out_info[p] > 0 gives NaN in out_logpdf[p], in
 * the particle's whole gradient block and in out_grad_noise[p]; the other particles of the call are untouched.  P == 0 is AGP_OK and
 * touches nothing.
 * The WHOLE call is rejected with
 *   AGP_ERR_ARG: everything agp_logpdf_series_batch lists, a null out_grad when prm_off[P] > 0, a null out_grad_noise;
 *   AGP_ERR_PROGRAM (names the particle): a malformed program; a tree of more than 64 nodes (agp_logpdf_grad_batch's limit); a
 *     particle whose LDS need under the gradient kernel's map exceeds 160 KiB at its series' length.  That map holds, beside the
 *     value kernel's arrays, a second 2 KiB table per ChangePoint node (1 - sigma, kept beside sigma for the derivatives' accuracy),
 *     alpha (8 bytes per padded point), the gradient program (8 bytes per node and per parameter) and the reduction scratch (32 bytes
 *     per parameter): at AGP_SERIES_MAX_N points a chain of 4 ChangePoint nodes (9 nodes, 13 parameters,
 *     4 per-point tables) fits and one of 5 does not, where the value entry takes 10.
 * Stateless and re-entrant like agp_logpdf_series_batch: needs no agp_set_data; leaves alone the resident series, the factor store and
 * its statistics, the gradient-reuse, lag-domain, Toeplitz and structured counters, the coalescer, dedup and mixture counters; copies
 * of a particle are NOT deduplicated; with profiling on agp_get_timing reports as for the value entry (out[0] = out[2] = the call's
 * kernel time).  A particle's result bits depend only on its own series, program, parameters and noise — not on what else is in the
 * call, its order, or how the call is split into launches. */
int agp_logpdf_grad_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                 int32_t P, const int32_t* series /* P */,
                                 const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                 const double* noise,
                                 double* out_logpdf /* P */, double* out_grad /* prm_off[P] */,
                                 double* out_grad_noise /* P */, int32_t* out_info /* P */);

/* HMC rejuvenation of many short series in one call: rejuvenate_particle_parameters (src/inference_smc_anneal_data.jl:33-76) for every
 * (series, particle) pair — per iteration one Gen.hmc move on all numeric kernel parameters, then one on the noise.  One workgroup
 * runs the whole chain of a particle: every evaluation is agp_logpdf_grad_series_batch's kernel body in a loop, with the state in LDS.
 * Series, program and info conventions are those of agp_logpdf_series_batch; there is no prm / noise argument — the state is latent.
 *
 * STATE.  Every moving parameter is z ~ N(0, 1) and theta = transform(z) (src/Model.jl:24-49).  tf[C][3] = (mu, sigma, scale) is the
 * table of transform classes: scale == 0 is log-normal, theta = exp(mu + sigma z); scale > 0 is logit-normal,
 * theta = scale / (1 + exp(-(mu + sigma z))).  prm_class[prm_off[P]] gives every caller parameter its class; a value < 0 means FIXED:
 * the slot of z holds the parameter value itself, it is not moved, has no prior term and comes back bit-identical (the reference's
 * ChangePoint scale).  noise = transform(z_noise[p]; tf[noise_class]) + noise_jitter (the reference's JITTER, 1e-5).
 * TARGET.  U = logpdf(xs_s; theta, noise) - 1/2 sum_selected z^2;  dU/dz_i = -z_i + (d logpdf / d theta_i)(d theta_i / d z_i), with
 * d theta / d z = sigma theta (log-normal), sigma theta (1 - theta / scale) (logit-normal), sigma (noise - noise_jitter) (noise).
 * ONE MOVE (Gen.hmc): value and gradient at the current state; momenta m; K0 = -1/2 sum m^2; L times { m += (eps/2) g; z += eps m;
 * value and gradient; m += (eps/2) g }; alpha = (U_new - U_0) + (K_new - K_0); accepted iff log u < alpha.  The parameter move
 * selects every parameter of class >= 0 (L_param, eps_param), the noise move z_noise alone (L_noise, eps_noise; skipped when
 * L_noise == 0).  A trajectory on which a pivot fails, or the value, a gradient component of the selection or a transformed parameter
 * is not finite, is rejected (alpha = -inf) and counted as not positive definite.
 * ITERATIONS.  i = 0 .. n_hmc - 1: parameter move, noise move, exit check — the particle stops after n_exit consecutive rejected
 * parameter moves (n_exit <= 0: never); the noise move of the stopping iteration still runs.  A particle without a moving parameter
 * makes no parameter move and its rejection counter never advances.
 * RANDOMNESS.  Philox4x64-10 under the key (seeds[p], 0), counter (c0 = block, c1 = i, c2 = move: 0 parameters / 1 noise,
 * c3 = 0x484D43).  The momentum of the k-th selected coordinate, in caller order, is ndtri(uniform(word k % 4 of block k / 4)); u is
 * uniform(word 0 of block 2^32) (uniform as in agp_predict_sample_batch).  Not Julia's stream.  A particle's chain depends on its
 * seed and its own inputs only: not on the batch, the order, copies, or how the call is split into launches.
 *
 * OUTPUTS.  out_z (layout prm_off), out_z_noise[P]: the final state.  out_prm: the transformed parameters of the final state in the
 * caller's order (fixed slots copied), out_noise[P].  out_logpdf[p] is bit-identical to what agp_logpdf_series_batch returns for
 * (out_prm, out_noise).  out_counts[P][4]: parameter moves accepted, parameter moves tried, noise moves accepted, trajectories
 * rejected as not positive definite.  out_trace[P][n_hmc][2][2] (or NULL): (alpha, log u) of every move, NaN for a move not made.
 * INITIAL STATE NOT POSITIVE DEFINITE: out_info[p] = k, out_logpdf[p] = NaN, out_z / out_z_noise the inputs, out_prm / out_noise their
 * transforms, no move; the other particles are untouched.  n_hmc == 0: the transformed inputs and their log-density.  A particle on
 * an EMPTY series is returned unmoved (transformed inputs, logpdf 0): moves under the prior alone are not made.  P == 0 is AGP_OK.
 * flags: bit 0 (measurement) makes noise moves run the whole gradient pass instead of d/d noise = 1/2 (alpha'alpha - |L^-T|_F^2).
 * The WHOLE call is rejected with
 *   AGP_ERR_ARG: everything agp_logpdf_grad_series_batch lists; a null output other than out_trace; a class index >= C (names the
 *     particle); a class with sigma <= 0 or scale < 0; noise_class outside [0, C); negative n_hmc, L_param, L_noise, eps_param, eps_noise;
 *   AGP_ERR_PROGRAM (names the particle): a malformed program, a tree of more than 64 nodes, or a particle whose LDS need under the
 *     HMC kernel's map exceeds 160 KiB: the gradient kernel's map plus six doubles per parameter (the caller-order vector, z, saved z,
 *     momentum, gradient, class and slot map), the class table and 32 doubles of chain state.  At AGP_SERIES_MAX_N points a chain of 4
 *     ChangePoint nodes still fits and one of 5 does not, as in the gradient entry.
 * Stateless and re-entrant like the other series entries. */
int agp_hmc_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                         int32_t P, const int32_t* series /* P */,
                         const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off,
                         const double* z /* prm_off[P] */, const double* z_noise /* P */, const int32_t* prm_class /* prm_off[P] */,
                         int32_t C, const double* tf /* C x 3 */, int32_t noise_class, double noise_jitter,
                         int32_t n_hmc, int32_t L_param, double eps_param, int32_t L_noise, double eps_noise, int32_t n_exit,
                         const uint64_t* seeds /* P */, int32_t flags,
                         double* out_z /* prm_off[P] */, double* out_z_noise /* P */, double* out_prm /* prm_off[P] */,
                         double* out_noise /* P */, double* out_logpdf /* P */, int32_t* out_counts /* P x 4 */,
                         int32_t* out_info /* P */, double* out_trace /* P x n_hmc x 2 x 2, or NULL */);

/* Forecasts of many short series in one call: agp_logpdf_series_batch's predictive twin (predict / predict_mvn, src/api.jl:497-596, on
 * the predictive of src/GP.jl:731-758) for callers that hold one model per short series.  The workgroup that has just factored
 * K11 = K_p(ts_s) + noise[p] I in LDS evaluates the cross-covariance K21 at the series' own query times 16 at a time and solves it
 * against that factor in registers; nothing but the outputs leaves the compute unit.
 * Series s has the training points [pt_off[s], pt_off[s+1]) and the m_s query times ts_pred[q_off[s] .. q_off[s+1]), which may repeat
 * and may coincide with training times (WhiteNoise is decided by time equality, as everywhere).  Particle p predicts on series[p]:
 *   mean = K21 K11^-1 x,   var = diag(K22 - K21 K11^-1 K12) + noise_pred[p]       (noise_pred NULL: noise)
 * — the marginal part of agp_predict_batch with zero mean functions; no full covariance here.
 * Output layout, particle-major: the entry writes out_off[p] = sum_{p' < p} m_{series[p']} (P + 1 values); particle p's m means and
 * variances start at out_off[p]; out_mean and out_var hold out_off[P] doubles each (the caller can size them from q_off and series).
 * Adjacent particles of one series therefore form the (P_s, m_s) row-major block that agp_mixture_quantile and agp_mixture_moments
 * take as is.
 * out_logpdf (P, or NULL): the training log marginal likelihood, bit-identical to agp_logpdf_series_batch's for the same particle.
 * Program encoding, noise meaning, out_info, AGP_SERIES_MAX_N, statelessness, re-entrancy, no deduplication and profiling timing are
 * exactly those of agp_logpdf_series_batch.  A series without query points (m_s == 0): nothing is written to out_mean / out_var for
 * its particles; out_logpdf and out_info are still set.  An EMPTY series with query points gives the prior predictive: mean 0,
 * var = k(t*, t*) + noise_pred, logpdf 0, info 0.  out_info[p] > 0 gives NaN in the particle's whole mean and variance block and in
 * out_logpdf[p]; the other particles are untouched.  A computed variance that is not positive (cancellation in K22 - K21 K11^-1 K12
 * when noise_pred does not lift it) is returned as computed — neither clamped nor reported — exactly as agp_predict_batch's out_var.
 * P == 0 is AGP_OK and touches nothing.
 * The WHOLE call is rejected with
 *   AGP_ERR_ARG (names the series or particle): everything agp_logpdf_series_batch lists, q_off[0] != 0, a decreasing q_off, a series
 *     with more than 2^30 query points, a null q_off, ts_pred, out_mean, out_var or out_off;
 *   AGP_ERR_PROGRAM (names the particle): as agp_logpdf_series_batch.  The predictive kernel's LDS map is the value kernel's (the
 *     solved query blocks live in registers, the ChangePoint tables' unused tail holds the query times' entries): at AGP_SERIES_MAX_N
 *     points a chain of 10 ChangePoint nodes (21 nodes, 31 parameters, 10 per-point tables) fits and one of 11 does not, as for the
 *     value entry.
 * A particle's result bits depend only on its own series, queries, program, parameters and noises — not on what else is in the call,
 * its order, or how the call is split into launches. */
int agp_predict_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                             const int64_t* q_off /* S+1 */, const double* ts_pred,
                             int32_t P, const int32_t* series /* P */,
                             const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                             const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                             double* out_mean, double* out_var, int64_t* out_off /* P+1 */,
                             double* out_logpdf /* P or NULL */, int32_t* out_info /* P */);

/* Forecast BANDS of many short series in one call: predict_quantile (src/api.jl:547-596) and the mixture mean of predict_mvn for
 * callers that hold one model per short series — agp_predict_series_batch followed, on the device and on the same stream, by the
 * read-out of every series' own mixture; what comes back is the band, not the P*m per-particle means and variances, and the call
 * synchronises once.  The resident-series twin is agp_predict_quantile_batch.
 * Predictive: exactly agp_predict_series_batch — arguments S .. noise_pred, validation and messages, LDS classes and launches, the
 *   noise_pred rule, the prior predictive of an empty series; out_logpdf (P, or NULL) is bit-identical to that entry's.
 * Mixture of series s: the particles p with series[p] == s, in ascending p (they need not be adjacent), with weights[p] — the weights
 *   of ONE series are finite, >= 0 and sum to 1 (rtol sqrt(eps)), as agp_mixture_quantile asks of its own.  A series without a
 *   particle is no error: its outputs are NaN, converged and iterations 0.
 * Raw space: agp_predict_quantile_batch's transform with the series' own (y_slope[s], y_intercept[s]) (NULL: 1 and 0):
 *   mu_raw = (mu - b) / a, var_raw = (1 / (a a)) var, 1 / (a a) formed once in double.
 * out_info[p]: the predictive's word; where that is 0 and a raw mean is not finite or a raw variance negative or NaN, n_s + i + 1 for
 *   the first such query i (0-based).  If ANY particle of a series has info != 0 — whatever its weight — that series' x and moments
 *   are NaN, its converged flags and iteration counts 0; every other series' bits are untouched.
 * Quantiles: 0 < q[k] < 1.  Series s's block of out_x starts at nq * q_off[s] and is (nq, m_s) row-major — agp_mixture_quantile's
 *   layout per series — out_converged and out_iters (nullable) likewise; its bits are those of agp_mixture_quantile(tol, max_iter) on
 *   the series' stacked (P_s, m_s) raw components (one search kernel body serves both).  nq == 0 is valid: moments only.
 * Moments: out_mix_mean / out_mix_var (q_off[S] each, nullable) at q_off[s] + i: the marginal mean and variance of the raw-space
 *   mixture (space 0 only), the bits of agp_mixture_moments on the stacked block: sums about the first component of positive weight,
 *   sequentially in particle order, weight-0 components skipped.
 * Device: a ragged pack kernel (transform, correctly rounded sqrt, one padded row per (series, query), info words), one wave per
 *   (series, query, quantile) for the searches, one thread per (series, query) for the moments; every word they read was written
 *   by the same call.  With profiling on, agp_get_timing's out[0] = out[2] = the predictive kernels as for agp_predict_series_batch
 *   and out[4] = the three read-out kernels together.
 * Stateless and re-entrant exactly as agp_predict_series_batch.  A series' result bits depend only on its own data, queries,
 *   particles (in their order), weights, transform, q, tol and max_iter — not on the other series, their order, or nq.
 * The WHOLE call is rejected, and nothing is written to any output, with everything agp_predict_series_batch reports, and with
 *   AGP_ERR_ARG: the weights of one series not finite, negative or not summing to 1, a y_slope that is 0 or not finite, an
 *   y_intercept that is not finite (each message names the series); q[k] outside (0, 1); nq < 0; a NULL weights, q (nq > 0) or out_x
 *   (nq > 0); nq * q_off[S] or sum_s m_s * ceil(P_s / 64) * 64 at or above 2^31. */
int agp_predict_quantile_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                      const int64_t* q_off /* S+1 */, const double* ts_pred,
                                      int32_t P, const int32_t* series /* P */,
                                      const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                      const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                      const double* weights /* P: particle p's weight inside ITS series' mixture */,
                                      const double* y_slope /* S, or NULL: 1 */, const double* y_intercept /* S, or NULL: 0 */,
                                      const double* q, int64_t nq, double tol, int64_t max_iter,
                                      double* out_x /* nq * q_off[S] */, int32_t* out_converged /* or NULL */,
                                      int32_t* out_iters /* or NULL */,
                                      double* out_mix_mean /* q_off[S], or NULL */, double* out_mix_var /* q_off[S], or NULL */,
                                      double* out_logpdf /* P, or NULL */, int32_t* out_info /* P */);

/* agp_predict_series_batch for series of up to AGP_LONG_SERIES_MAX_N = 512 points: the forecast of the reference's 442-point data
 * set beside its 135- and 143-point ones in ONE call.  The arguments are agp_predict_series_batch's with a trailing flags word, and
 * every convention is that entry's: the particle-major layout behind out_off, noise_pred NULL = noise, the optional out_logpdf,
 * nothing written for a series with m_s == 0, the prior predictive of an EMPTY series, NaN in the whole block and in out_logpdf of
 * a particle with out_info[p] > 0 (the first non-positive pivot), a variance neither clamped nor reported, P == 0, the error
 * codes and their messages (the cap now AGP_LONG_SERIES_MAX_N, named in the message); flag bits other than AGP_LONG_SERIES_ALL are
 * AGP_ERR_ARG.  Stateless and re-entrant like it.
 * Routing, as in agp_logpdf_long_series_batch: a series of at most AGP_SERIES_MAX_N points (an empty one always) runs in
 * agp_predict_series_batch's kernel, bit-identical to that entry; a longer one runs in k_long_series_predict — the long value
 * kernel's statements, then, in the same workgroup, the posterior at the series' own query times: query blocks of 16 times dealt to
 * the four waves, solved block column by block column against the factor in the workspace (v_mfma_f64_16x16x4), the solved blocks
 * in scratch rows of that workspace.  flags & AGP_LONG_SERIES_ALL sends every non-empty series through it.  out_logpdf is
 * bit-identical to agp_logpdf_long_series_batch's under the same flags.
 * Workspace: from the call's slot, 852 blocks of 2 KiB (1.66 MiB) per workgroup at 512 points whatever m_s is; one launch takes at
 * most min(agp_set_workspace_limit's value, 1 GiB) and a larger call is split into launches on its stream.  A particle's result
 * bits depend only on its own series, program, parameters, noises and the flag, and a query's only on its own time beside them —
 * not on the other query times, their number or order, on what else is in the call, or on the split.
 * AGP_ERR_PROGRAM (names the particle): the long predictive kernel keeps 5 KiB per ChangePoint node (640 table entries: 512 points
 * and 128 query slots) beside 21.5 KiB and the program: at 512 points a chain of 10 ChangePoint nodes takes 71.5 KiB (two workgroups
 * still share a CU); 27 nodes beside a small program are the most 160 KiB hold. */
int agp_predict_long_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                  const int64_t* q_off /* S+1 */, const double* ts_pred,
                                  int32_t P, const int32_t* series /* P */,
                                  const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                  const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                  double* out_mean, double* out_var, int64_t* out_off /* P+1 */,
                                  double* out_logpdf /* P or NULL */, int32_t* out_info /* P */, uint32_t flags);

/* The forecast BAND for series of up to AGP_LONG_SERIES_MAX_N points: agp_predict_quantile_series_batch's arguments with a trailing
 * flags word.  The predictive launches are agp_predict_long_series_batch's (routing, workspace, splitting, flags, refusals); behind
 * them the pack, search and moment kernels of agp_predict_quantile_series_batch run unchanged on the same stream, so a series' band
 * has the bits of agp_mixture_quantile / agp_mixture_moments on the raw components of that entry's block, and every mixture rule,
 * output layout and refusal is agp_predict_quantile_series_batch's.  A series with a failed particle is NaN; the others are
 * untouched. */
int agp_predict_quantile_long_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                           const int64_t* q_off /* S+1 */, const double* ts_pred,
                                           int32_t P, const int32_t* series /* P */,
                                           const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                           const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                           const double* weights /* P: particle p's weight inside ITS series' mixture */,
                                           const double* y_slope /* S, or NULL: 1 */, const double* y_intercept /* S, or NULL: 0 */,
                                           const double* q, int64_t nq, double tol, int64_t max_iter,
                                           double* out_x /* nq * q_off[S] */, int32_t* out_converged /* or NULL */,
                                           int32_t* out_iters /* or NULL */,
                                           double* out_mix_mean /* q_off[S], or NULL */, double* out_mix_var /* q_off[S], or NULL */,
                                           double* out_logpdf /* P, or NULL */, int32_t* out_info /* P */, uint32_t flags);

/* HELD-OUT SCORES of many short series in one call: predict_proba (src/api.jl:686-699) for callers that hold one model per short
 * series — the log-density of every series' held-out values y_pred under each of its particles' posterior predictives, and (with
 * weights) under every series' own mixture.  The resident-series twin is agp_predict_logpdf_batch, and the route is that entry's: one
 * workgroup per particle factors the JOINT matrix [K11 + noise I, K12; K21, K22 + noise_pred I] of the series' n_s training points
 * followed by its m_s query points — a short series of N = n_s + m_s <= AGP_SERIES_MAX_N points, in agp_logpdf_series_batch's kernel
 * body and LDS map at N points — and reads the query rows' partials: with L the joint factor and z = L^-1 [xs; y_pred],
 *   out_logpdf[p] = -(m log 2pi + 2 sum_{k >= n} log L_kk + sum_{k >= n} z_k^2) / 2 + m log|y_slope[s]|.
 * Arguments S .. noise_pred as agp_predict_series_batch (series s is scored at ts_pred[q_off[s] .. q_off[s+1]); query times may
 * repeat and may coincide with training times; noise_pred NULL: each particle's noise).  y_pred: q_off[S] values ALREADY in the
 * transformed space, as xs is.  y_slope (S, or NULL: 1) enters through the Jacobian term alone: the result is the log-density of the
 * RAW values (y_pred - intercept) / slope.
 * out_terms (out_off[P] doubles, or NULL), particle-major behind out_off as in agp_predict_series_batch (out_off: P + 1, or NULL):
 *   out_terms[out_off[p] + j] = -(log 2pi + z_{n+j}^2) / 2 - log L_{n+j,n+j} + log|y_slope[s]|, the log-density of held-out point j
 *   given the training data and the held-out points before it in the caller's order (the prequential score); they sum to out_logpdf[p].
 * out_info[p] (agp_predict_logpdf_batch's convention): 0, or the first bad pivot of the joint factor — 1 .. n_s when K11 fails,
 *   n_s + k when leading minor k of the predictive covariance fails; NaN is then in out_logpdf[p] and in the particle's whole block of
 *   out_terms, and no other particle is affected.  An empty training series gives the prior predictive's density.  A particle whose
 *   series has nothing held out (m_s == 0) is not launched: logpdf 0, info 0.
 * Mixtures (weights: P values, particle p's weight inside ITS series' mixture; NULL: none, and out_series_logp must then be NULL too):
 *   out_series_logp[s] = M + log sum_{w_p > 0} w_p exp(out_logpdf[p] - M), M = max_{w_p > 0} out_logpdf[p], over the particles p with
 *   series[p] == s in ascending p (they need not be adjacent) — the log of predict_mvn's mixture density at the held-out vector, raw
 *   space — formed on the device behind the kernels, one thread per series.  If ANY particle of a series has info != 0, whatever
 *   its weight, that series' value is NaN and every other series' is untouched; a series with particles and m_s == 0 gives exactly
 *   0.0; a series without particles gives NaN and is no error (agp_predict_quantile_series_batch's rule).
 * Stateless and re-entrant exactly as agp_predict_series_batch: one upload, one synchronisation.  A particle's result bits depend
 *   only on its own series, queries, held-out values, program, parameters, noises and slope; a series' mixture bits only on its own
 *   particles (in their order) and weights.  With profiling on, agp_get_timing's out[0] = out[2] = the fused kernels and out[4] = the
 *   mixture read-out.
 * The WHOLE call is rejected, and nothing is written to any output, with everything agp_predict_series_batch reports, and with
 *   AGP_ERR_ARG (each message names the series): a series with m_s > 0 and n_s + m_s > AGP_SERIES_MAX_N (both counts are given); a
 *     NULL y_pred when q_off[S] > 0; a held-out value that is not finite; a y_slope that is 0 or not finite; the weights of one series
 *     not finite, negative or not summing to 1 (rtol sqrt(eps)); weights / out_series_logp not both NULL or both given;
 *   AGP_ERR_PROGRAM (names the particle): a particle whose LDS need at N = n_s + m_s points exceeds 160 KiB — at N = AGP_SERIES_MAX_N
 *     a chain of 10 ChangePoint nodes fits and one of 11 does not, as in agp_logpdf_series_batch at that length.
 * Not here: the m x m predictive covariance, mean functions, n_s + m_s > AGP_SERIES_MAX_N (agp_predict_logpdf_long_series_batch
 * below takes up to AGP_LONG_SERIES_MAX_N), deduplication inside a call. */
int agp_predict_logpdf_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                    const int64_t* q_off /* S+1 */, const double* ts_pred, const double* y_pred /* q_off[S] */,
                                    int32_t P, const int32_t* series /* P */,
                                    const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                    const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                    const double* y_slope /* S, or NULL: 1 */, const double* weights /* P, or NULL */,
                                    double* out_logpdf /* P */, double* out_terms /* out_off[P], or NULL */,
                                    int64_t* out_off /* P+1, or NULL */, double* out_series_logp /* S; NULL iff weights is */,
                                    int32_t* out_info /* P */);

/* agp_predict_logpdf_series_batch for n_s + m_s of up to AGP_LONG_SERIES_MAX_N = 512 JOINT points: the reference tutorial's split of
 * 144 training + 36 held-out points (180) and held-out tails of its 442-point data set, beside the short series, in ONE call.  The
 * arguments are agp_predict_logpdf_series_batch's with a trailing flags word, and every convention is that entry's: y_pred in the
 * space of xs, y_slope through the Jacobian term alone, noise_pred NULL = noise, the optional out_terms behind out_off, out_info on
 * the JOINT index (1 .. n_s when K11 fails, n_s + k for leading minor k of the predictive covariance; NaN then in out_logpdf[p] and
 * in the particle's whole block of out_terms), the prior predictive's density for an empty training series, logpdf 0 / info 0
 * without a launch where m_s == 0, the mixtures' rules (k_series_mix_logp runs unchanged behind the launches on the same stream),
 * P == 0, one upload and one synchronisation, agp_get_timing's words, the error codes and their messages.  Stateless and
 * re-entrant like it.
 * Routing by the JOINT length N = n_s + m_s, as in agp_logpdf_long_series_batch by n_s: N <= AGP_SERIES_MAX_N runs in
 * agp_predict_logpdf_series_batch's kernel, bit-identical to that entry (logpdf, terms, mixtures, info); a longer one runs in
 * k_long_series_predict_logpdf — the long value kernel's statements on the joint points with the two-noise diagonal, its two
 * reductions restricted to the query rows [n_s, N) — in the long value kernel's LDS map and workspace at N points.
 * flags & AGP_LONG_SERIES_ALL sends every particle with m_s > 0 through it.  With n_s == 0, y_slope NULL and noise_pred NULL,
 * out_logpdf is bit-identical to agp_logpdf_long_series_batch's on the series (ts_pred, y_pred) under the same flags.
 * Workspace: from the call's slot, 528 blocks of 2 KiB (1.03 MiB) per workgroup at 512 joint points; one launch takes at most
 * min(agp_set_workspace_limit's value, 1 GiB) and a larger call is split into launches on its stream.  A particle's result bits
 * depend only on its own series, queries, held-out values, program, parameters, noises, slope and the flag — not on what else is
 * in the call, its order, or the split.
 * The WHOLE call is rejected, and nothing is written to any output, with everything agp_predict_logpdf_series_batch reports, where
 *   AGP_ERR_ARG: a series of more than AGP_LONG_SERIES_MAX_N training points; a series with m_s > 0 and n_s + m_s >
 *     AGP_LONG_SERIES_MAX_N (the message names the series, both counts and that constant); flag bits other than AGP_LONG_SERIES_ALL;
 *   AGP_ERR_PROGRAM (names the particle): a particle whose LDS need at N joint points exceeds 160 KiB.  On the long route that is
 *     the long value kernel's need, 21 KiB + the program + 4 KiB per ChangePoint node at N = 512: a chain of 10 ChangePoint nodes
 *     takes 61 KiB, one of 34 is the longest that fits and one of 35 is refused.
 * Not here: the sampling, gradient, decomposition and HMC twins above AGP_SERIES_MAX_N points; the m x m predictive covariance;
 * mean functions; n_s + m_s > AGP_LONG_SERIES_MAX_N; deduplication inside a call. */
int agp_predict_logpdf_long_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                         const int64_t* q_off /* S+1 */, const double* ts_pred, const double* y_pred /* q_off[S] */,
                                         int32_t P, const int32_t* series /* P */,
                                         const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                         const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                         const double* y_slope /* S, or NULL: 1 */, const double* weights /* P, or NULL */,
                                         double* out_logpdf /* P */, double* out_terms /* out_off[P], or NULL */,
                                         int64_t* out_off /* P+1, or NULL */, double* out_series_logp /* S; NULL iff weights is */,
                                         int32_t* out_info /* P */, uint32_t flags);

/* SAMPLE PATHS and JOINT FORECASTS of many short series in one call: rand(predict_mvn(model, ds), R) and the components of
 * predict_mvn's MixtureModel (src/api.jl:497-522) for callers that hold one model per short series.  The resident-series twins are
 * agp_predict_sample_batch and agp_predict_batch(want_cov); the route is agp_predict_logpdf_series_batch's: one workgroup per
 * particle factors the joint matrix of the series' n_s training points followed by its m_s query points with a zero query right-hand
 * side, after which the query rows of the factor are [L21 L22] with L22 = chol(Sigma*) and a = L11^-1 xs, and everything is a
 * read-out of those rows in the same workgroup: mu* = L21 a, Sigma* = L22 L22', x = mu* + L22 z.
 * Arguments S .. noise_pred as agp_predict_logpdf_series_batch, without y_pred.  y_slope / y_intercept (S each, or NULL: 1 / 0): the
 * transform of series s (scaled = slope raw + intercept); every output is in RAW space.  weights (P): particle p's weight inside ITS
 * series' mixture (the particles of a series need not be adjacent).  R >= 0 samples per series, the same for every series; R == 0:
 * only out_mean / out_cov / out_info are produced.
 * Draws: series s draws exactly as agp_predict_sample_batch does under seed = seeds[s] — Philox4x64-10 under the key (seeds[s], 0);
 *   the component of sample j from the uniform of word 0 of block (j, 0, 0, 0) through the inverse CDF of the cumulative weights of
 *   the series' particles in ascending p; the uniform of z[j, i] is word i % 4 of block (i / 4, j, 1, 0); normals by ndtri.
 *   component (S R int32, or NULL): global particle indices, sample j of series s at s R + j; each must be a particle of series s of
 *   positive weight.  z (R q_off[S] doubles in out_x's layout, or NULL): they replace the normal draws.  seeds may be NULL only when
 *   nothing is left to draw.
 * out_x (R q_off[S] doubles): series s owns [R q_off[s], R q_off[s+1]); sample j is the column of m_s values at + j m_s:
 *   x = (mu*_c - b_s) / a_s + (L22_c z_j) / |a_s|, evaluated as (mu* + sign(a_s) L22 z - b_s) / a_s (c the sample's component).
 * out_component (S R, or NULL): the components used.
 * out_mean (out_off[P] doubles, or NULL; out_off: P + 1, written by the entry, particle-major as in agp_predict_series_batch):
 *   (mu*_p - b) / a.  out_cov (cov_off[P] doubles, or NULL; cov_off: P + 1, written by the entry, the running sum of m_s^2):
 *   Sigma*_p / a^2, m_s x m_s column-major, both triangles written, exactly symmetric.  Together they are the components of
 *   predict_mvn's mixture for every series; adjacent particles of one series form the block agp_mixture_moments takes.
 * out_info[p]: agp_predict_logpdf_series_batch's convention (first bad pivot of the joint factor).  If ANY particle of a series has
 *   info != 0, whatever its weight, that series' whole block of out_x is NaN (the reference throws); the failed particle's own
 *   out_mean / out_cov blocks are NaN; no other series and no other particle changes a bit (the fill runs on the device behind the
 *   kernels, on the same stream).  m_s == 0 writes nothing for the series; n_s == 0 samples the prior K22 + noise_pred I.
 * Bit contract: the bits of sample j of series s depend only on seeds[s] (or the caller's z and component), j, and the inputs of its
 *   component — program, parameters, noises, the series, its queries, the transform.  They do not depend on R, on the other series or
 *   particles, on the order of the batch, or on which samples share a group of 16 on the device.  out_mean / out_cov depend on the
 *   particle's own inputs only.
 * Stateless and re-entrant as agp_predict_series_batch: one upload, one synchronisation; neither the resident series nor the factor
 *   store is touched.  With profiling on, agp_get_timing's out[0] = out[2] = the fused kernels and out[4] = the NaN-fill read-out.
 * The WHOLE call is rejected, and nothing is written to any output, with everything agp_predict_logpdf_series_batch reports (the cap
 *   n_s + m_s <= AGP_SERIES_MAX_N and the LDS need at that length included: 144 training points + 36 queries are 180 and refused),
 *   and with AGP_ERR_ARG (each message names the series): R < 0; R q_off[S] >= 2^31; a series without particles when R > 0; a
 *   component outside its series or of weight 0; a z that is not finite; a y_slope that is 0 or not finite or a y_intercept that is
 *   not finite; NULL weights, out_x (with something to write), seeds (with something to draw), out_off with out_mean, cov_off with
 *   out_cov.
 * Not here: mean functions, n_s + m_s > AGP_SERIES_MAX_N, deduplication inside a call. */
int agp_predict_sample_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                    const int64_t* q_off /* S+1 */, const double* ts_pred, int32_t P, const int32_t* series /* P */,
                                    const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                    const double* noise /* P */, const double* noise_pred /* P or NULL = noise */,
                                    const double* y_slope /* S, or NULL: 1 */, const double* y_intercept /* S, or NULL: 0 */,
                                    const double* weights /* P */, int64_t R, const uint64_t* seeds /* S */,
                                    const int32_t* component /* S R, or NULL */, const double* z /* R q_off[S], or NULL */,
                                    double* out_x /* R q_off[S] */, int32_t* out_component /* S R, or NULL */,
                                    double* out_mean /* out_off[P], or NULL */, int64_t* out_off /* P+1, or NULL */,
                                    double* out_cov /* cov_off[P], or NULL */, int64_t* cov_off /* P+1, or NULL */,
                                    int32_t* out_info /* P */);

/* DECOMPOSITIONS of many short series in one call: predict_sum / predict_mvn_sum's marginals (src/api.jl:898-1034 on GP.infer_gp_sum,
 * src/GP.jl:904-993) for callers that hold one model per short series — agp_predict_sum_batch's twin, on agp_predict_series_batch's
 * route: the workgroup that has factored K11 in LDS solves the coded query rows against it in registers and reads them out itself.
 * Arguments S .. ts_pred as agp_predict_series_batch.  Components: every particle has M >= 1 component kernels (split_kernel_sop
 * gives M = 2); particle p's are the CSR entries [p M, (p + 1) M) of op_off / prm_off (P M + 1 offsets each), as in
 * agp_infer_gp_sum_batch; its model is X = F_1 + .. + F_M + noise on series[p], evaluated as the ONE composite program
 * K_1 SEL_1 * K_2 SEL_2 * + .. on coded points.  noise / noise_pred (P; noise_pred NULL: noise) as agp_predict_series_batch.
 * y_slope / y_intercept (S each, or NULL: 1 / 0): the transform of series s (scaled = a_s raw + b_s).  q (nq >= 0 values in (0, 1)).
 * Rows: series s with m_s query times has (M + 1) m_s joint rows g in the reference's order F_1(T*) .. F_M(T*), X(T*); row g is
 *   component i = g / m_s at query time g % m_s.  Scaled posterior: mean = K21 K11^-1 x, var = (k** - |K21 L^-T|^2) + 1e-8, and
 *   + noise_pred[p] on the X rows only.  Returned are predict_sum's RAW numbers, formed as agp_predict_sum_batch forms them:
 *   out_mean = (mean - b_s) / a_s, + b_s / a_s on the F_1 rows (the intercept counted once); out_var = (1 / (a_s a_s)) var;
 *   out_x[row nq + k] = fma(sqrt(out_var), ndtri(q[k]), out_mean).
 * Output layout, particle-major: the entry writes out_off[p] = (M + 1) sum_{p' < p} m_{series[p']} (P + 1 values); particle p owns
 *   (M + 1) m_s means (and variances; out_var may be NULL) from out_off[p] and nq quantiles per row from nq out_off[p] (out_x: NULL
 *   iff nq == 0).  Adjacent particles of one series form the (P_s, (M + 1) m_s) block agp_mixture_quantile / agp_mixture_moments take.
 * out_logpdf (P, or NULL): the training log marginal likelihood of the summed model.  out_info[p]: the first bad pivot of K11 (NaN
 *   then in all of the particle's outputs), else n_s + g + 1 for the first row g whose raw variance is negative or NaN or whose raw
 *   mean is not finite (NaN then in the particle's whole mean / variance / quantile blocks), else 0; no other particle changes.
 * m_s == 0 writes nothing for the series' particles but out_logpdf / out_info; an EMPTY series with query points gives the prior of
 *   every part: mean 0, var_i = K_i(t, t) + 1e-8, X also + noise_pred.  P == 0 is AGP_OK and touches nothing.
 * Stateless and re-entrant as agp_predict_series_batch: one upload, one synchronisation; the resident series, the factor store and
 *   every counter are left alone; copies are not deduplicated.  A particle's bits depend only on its own series, queries, components,
 *   noises and transform — not on the rest of the call, its order, or how it is split into launches.
 * The WHOLE call is rejected, and nothing is written to any output, with everything agp_predict_series_batch reports, and with
 *   AGP_ERR_ARG: M < 1, malformed component offsets (names particle and component), nq < 0, a q[k] outside (0, 1) or NaN, a y_slope
 *     that is 0 or not finite or a y_intercept that is not finite (names the series), an output of 2^31 elements or more;
 *   AGP_ERR_PROGRAM (names the particle): an unknown opcode, a composite over AGP_MAX_OPS nodes, an evaluation stack deeper than 8, or
 *     per-point tables that do not fit the kernel's 160 KiB at the series' length — every selector takes one 2 KiB table like a
 *     ChangePoint node, so at AGP_SERIES_MAX_N points and M = 2 a composite with 8 ChangePoint nodes (23 nodes, 28 parameters,
 *     10 tables: 163 280 of 163 840 bytes) fits and one with 9 (165 376 bytes) does not; the predictive entry's limit there is 10.
 * Not here: mean functions, the joint covariance of the parts (predict_mvn_sum's full matrix), n_s > AGP_SERIES_MAX_N. */
int agp_predict_sum_series_batch(agp_ctx* ctx, int32_t S, const int64_t* pt_off /* S+1 */, const double* ts, const double* xs,
                                 const int64_t* q_off /* S+1 */, const double* ts_pred, int32_t P, int32_t M,
                                 const int32_t* series /* P */, const int32_t* op_off /* P*M+1 */, const uint8_t* ops,
                                 const int32_t* prm_off /* P*M+1 */, const double* prm, const double* noise /* P */,
                                 const double* noise_pred /* P or NULL = noise */, const double* y_slope /* S or NULL */,
                                 const double* y_intercept /* S or NULL */, const double* q, int64_t nq,
                                 double* out_mean, double* out_var /* or NULL */, double* out_x /* NULL iff nq == 0 */,
                                 int64_t* out_off /* P+1 */, double* out_logpdf /* P or NULL */, int32_t* out_info /* P */);

/* agp_logpdf_batch with BLOCK-EXTENSION of resident factors.  The data-annealing loop re-scores
 * every particle on a longer prefix of the same series with unchanged kernel parameters — the reweight step
 * (src/inference_smc_anneal_data.jl:206-217), add_data! (src/api.jl:426-443), scripts/online.jl:200 — and the
 * reference refactorises from scratch each time.  This entry keeps each particle's Cholesky factor (packed tiles,
 * per-column inverse blocks, forward-solve vector, log-det / quadratic-form partials) in a context-owned store keyed by
 * the exact bits of (program, parameters, noise).  Called again with a larger n for a particle it holds, it only
 * computes the tile rows from floor(n_cached / 128) on: L_new = [L_old 0; B L_old^-T, chol(C - ..)], i.e.
 * (n^3 - n_cached^3)/3 flops instead of n^3/3; called with the same n it only re-reads the result.  Results equal
 * agp_logpdf_batch's (same kernels, same operation order per tile).  Any change of a parameter bit or of the tree is a
 * different key and factors from scratch; agp_set_data keeps the store when the new series has the resident one as a
 * prefix (add_data! appends) and empties it otherwise.  Duplicate particles (resampled populations) are evaluated
 * once.  The store takes at most ~45 % of device memory, slots are recycled least-recently-used; a population that
 * cannot fit runs through agp_logpdf_batch unchanged.  One extension sweep at a time per context. */
int agp_logpdf_batch_extend(agp_ctx* ctx, int64_t n, int32_t P,
                            const int32_t* op_off, const uint8_t* ops,
                            const int32_t* prm_off, const double* prm,
                            const double* noise,
                            double* out_logpdf /* P */, int32_t* out_info /* P */);
/* out4 = { particles extended from a resident factor, particles factored from scratch,
 *          tile rows reused, tile rows a from-scratch sweep would have computed } since agp_init / the last reset */
int agp_extend_stats(agp_ctx* ctx, int64_t* out4);
/* The same and more, up to n_out <= 10 values: out[0..3] as agp_extend_stats; out[4] = evicted_before_reuse — lookups (extension,
 * gradient or predictive sweeps) whose factor HAD been resident and was dropped for room before anything started from it: the cliff
 * of a store too small for its population (the gradient call of a leapfrog step refactoring what the value call before it had just
 * computed).  0 in a healthy run; factors nobody comes back for (the last state of a move, rejected proposals) are not counted.  The
 * library remembers the last 8192 such keys.  out[5] = slots the store holds; out[6] = distinct threads seen by the single-particle
 * entries since the last agp_set_data of another series / agp_extend_reset; out[7] = occupied slots; out[8] = tile rows a slot can
 * hold; out[9] = resizes that copied resident factors into the new allocation (since the context was created). */
int agp_extend_stats2(agp_ctx* ctx, int64_t* out, int32_t n_out);
/* forget every resident factor (release_memory != 0 also frees the store) */
int agp_extend_reset(agp_ctx* ctx, int release_memory);

/* remove_data! (src/api.jl:449-468): delete observations from the resident series and keep the resident factors.
 * idx: k distinct positions (0-based, ascending) of the resident series, in the caller's order.  The survivors keep their order
 * (deleteat!); the reduced series goes through agp_set_data's own grid / lattice detection and tables.  A resident factor of prefix
 * n_f that contains removed positions is UPDATED on the device to the factor of the reduced prefix (n_f minus the removed positions
 * below n_f; a rank-r update of the trailing triangle per contiguous run, csrc/agp_remove_kernel.hpp), or dropped where refactoring
 * is cheaper (remove_admits, csrc/agp_host.hpp) — its key stays (program, parameters, noise), so agp_logpdf_batch_extend at the new
 * n (the reference's smc_step! after the deletion) starts from it; factors on prefixes below idx[0] are untouched.  An updated
 * factor agrees with a from-scratch one to rounding (1e-8 relative on the log-density), not to the bit; its resident L^-T is
 * released.  A factor whose updated diagonal is not finite and positive is dropped (the next sweep reports the particle's info).
 * AGP_ERR_ARG: k <= 0, positions unsorted, duplicate or out of range ("no such time points"); AGP_ERR_NODATA before agp_set_data.
 * Under reference arithmetic nothing is resident: the call only edits the series. */
int agp_remove_data(agp_ctx* ctx, const int64_t* idx, int64_t k);
/* up to n_out <= 4 values since agp_init: factors updated, factors dropped, rows removed, panel steps run */
int agp_get_remove_stats(agp_ctx* ctx, int64_t* out, int32_t n_out);
/* env AGP_REMOVE_UPDATE [1]; 0 = agp_remove_data always drops the factors it touches */
int agp_set_remove_update(agp_ctx* ctx, int32_t on);
/* pre-size the store for series of up to n_cap observations and n_slots particles.  OPTIONAL: the store sizes itself — twice the
 * largest batch to begin with, and from there DRIVEN BY PRESSURE: it grows (keeping its contents, within its 45 % share of device
 * memory) rather than evict a factor that is still waiting for its first use — stored within the last 64 sweeps, nothing has started
 * from it, and its caller (the thread of the single-particle entry that stored it) has not stored another one since.  agp_logpdf /
 * agp_logpdf_grad are coalesced into batches of whatever size the callers' arrival times give, while every thread's value factor waits
 * for its gradient call: sized by the batch alone, a population arriving in small batches evicted its own factors between update and
 * choice_gradients.  Eviction order: free slots, factors already started from / abandoned by their caller / aged out (least recently
 * used first), and only then waiting ones.  The growth by pressure is capped at twice what the batch and the callers seen ask for
 * (value calls nothing comes back for — rejected proposals — must not fill the store's whole share).  Reserving up front only saves
 * the growth copies of the first sweeps; callers that score a whole population BEFORE differentiating any of it from short-lived
 * threads (thread ids recycled) are the one pattern that still profits.  agp_extend_stats2 shows the outcome. */
int agp_extend_reserve(agp_ctx* ctx, int64_t n_cap, int32_t n_slots);
/* The predictive entries consult the same store: a particle whose factor of exactly the prefix n is resident (the
 * per-step callback of the streaming workload predicts right after the reweight: scripts/online.jl:43,59 ->
 * src/inference_utils.jl:174-196) takes L11, its inverse blocks and alpha = L11^-1 x from the store and only computes
 * the prediction rows — n^2 m (+ n m^2 with a covariance request) instead of n^3/3 + n^2 m (+ n m^2).  Not used with
 * a training mean function (alpha would differ).  AGP_PREDICT_REUSE=0 disables.
 * out2 = { particles predicted from a resident factor, particles whose K11 was factored by the predictive pass } */
int agp_predict_reuse_stats(agp_ctx* ctx, int64_t* out2);
/* The single-particle entry agp_logpdf (coalesced inside the library) leaves its factors in the same store by default
 * (AGP_FACTOR_CACHE=0 / agp_set_factor_cache(ctx, 0) restore plain sweeps), which gives Gen's own call sequences the
 * reuse without any change on the Julia side:
 *   - the reweight step scores every particle again on a longer prefix with unchanged parameters
 *     (src/inference_smc_anneal_data.jl:127-141,206-217): an extension sweep;
 *   - each leapfrog step of Gen.hmc is `update` (a value call) followed by `choice_gradients` at the SAME parameters
 *     (src/inference_smc_anneal_data.jl:63-67): agp_logpdf_grad / agp_logpdf_grad_batch find the factor resident and
 *     start at L^-T — the covariance build and the n^3/3 factorisation are not repeated;
 *   - a value call repeated at unchanged parameters costs a lookup.
 * Results are those of the from-scratch sweeps to rounding (the resident factor may come from a chain of extension
 * sweeps, whose tiles are bit-identical to a from-scratch sweep of the same entry).
 * out2 = { particles of gradient sweeps served from a resident factor, particles factored by the gradient sweep } */
int agp_grad_reuse_stats(agp_ctx* ctx, int64_t* out2);
int agp_set_factor_cache(agp_ctx* ctx, int32_t on);

/* Regular time grids.  agp_set_data checks whether the series' time points, put in ascending order, are equally spaced
 * (every point within 1e-11 SPACINGS of t_0 + g h, one ulp of |t|max included: np.linspace, range(...), a min-max rescaled
 * daily / hourly / yearly index; a grid with an offset of 1e3 spacings-per-ulp or more — linspace(1000, 1001, 2048) — or a jitter
 * above that bound takes the general path, because the tables replace t_i - t_j by a representative of the lag).  If
 * so, value sweeps over the WHOLE series (n == n_max; agp_logpdf_batch{,_device,_multi}) run on a sorted copy of the data
 * — log N(x; 0, K) is invariant under a symmetric permutation of K and x — where an element of a tile depends on
 * (row - column) only: every stationary leaf (SquaredExponential, GammaExponential, Periodic; src/GP.jl:236-245,
 * 279-289, 324-336) is evaluated 255 times per 128 x 128 tile into an LDS table instead of 16 384 times, and tiles are
 * evaluated inside the factorisation kernels whatever the kernel tree's size.  Results agree with the general path to
 * rounding (the table's representative t_i - t_j differs from an element's own by a few ulp of t).  Prefix sweeps
 * (n < n_max: a subset of a shuffled grid is not a grid), gradient sweeps and the factor store's sweeps use rank tables instead
 * (below), predictive passes on lattice query points too; irregular series take the general path.  AGP_LAG=0 / agp_set_lag_tables(ctx, 0) disable it.  Of
 * agp_set_lag_tables, the admission part (0 / non-zero) is read at the next agp_set_data; the sweeps also test the switch, so 0
 * takes effect at once, and the levels 2 / 3 (structured value sweep, below) apply from the next sweep.  agp_get_lag_stats: whether the resident series qualifies, and how many sweeps took the path. */
int agp_get_lag_stats(agp_ctx* ctx, int32_t* regular_grid, int64_t* n_lag_sweeps);
int agp_set_lag_tables(agp_ctx* ctx, int32_t on);

/* Lattices with gaps: business-day indices, short calendar indices, regular series with missing observations.  The reference turns
 * dates into seconds (datetime2unix, src/api.jl:49-51) and min-max rescales them (src/api.jl:98-101); a business-day index (gaps of
 * 1 and 3 days), month starts (28..31 days) or a daily / hourly series with missing observations are not regular grids, but every
 * such time point is t_0 + g h with an INTEGER g, i.e. |t_a - t_b| = |g_a - g_b| h for every pair, which is all the rank tables
 * below need.  When the regular-grid test fails, agp_set_data looks for the largest h = (smallest gap) / k, k <= 400, that puts every
 * sorted point within 1e-11 SMALLEST GAPS of t_0 + g h, for spans of up to 4096 lattice points (the LDS budget of a rank table;
 * n_lattice <= n^2 / 2): the series' "ranks" are then the lattice indices g_i, a stationary subtree's table holds n_lattice lags, and
 * every caller-order sweep — value, prefix, factor store, gradient factorisation, predictive passes on lattice query points — takes
 * the table-driven evaluator.  The sorted sweeps with per-tile tables, the Toeplitz paths and the lag-domain gradient need
 * CONSECUTIVE lattice points and stay with regular grids.  Longer lattices (2048 month starts span 62 304 days) keep the general
 * evaluator: their tables would be gathered from L2, which was measured slower than evaluating the leaves (NOTES_dead_ends.md,
 * round 5).  agp_get_lattice_stats: kind = 0 (general path), 1 (regular grid), 2 (lattice with gaps), 3 (a longer lattice served by
 * COMPACT tables, below); AGP_LATTICE=0 / agp_set_lattice(ctx, 0) admit regular grids only (read at the next agp_set_data).
 *
 * Compact tables (kind 3; round 6): the reference's flagship series are monthly (docs/src/tutorials/assets/tsdl.161.csv through
 * src/api.jl:49-51,98-101) and a table over the lattice LAGS of 135 or more month starts exceeds the 4096 entries above.  In time
 * order, though, the lattice lag of a pair (i, i + od) of such a series takes only a few values — month starts: at most 5 whatever
 * od, quarters 4, years 2 — so a stationary subtree's table is indexed by (ordinal difference od, lattice lag - base[od]) and holds
 * W n entries, W = the largest number of distinct lags at one ordinal difference (admitted up to 8, n <= 4096, spans below 2^19
 * lattice points; the same position bound as above).  While W n <= 4096 the whole table sits in the evaluators' LDS and every value /
 * factorisation sweep in the CALLER's order reads it (batch, prefix, factor store, the factorisation of a gradient sweep): 819 month
 * starts, 68 years of monthly data.  Longer series (2048 month starts: 10 240 entries) use them on agp_logpdf_batch's sorted sweep over
 * the whole series, where a tile needs the window of its 256 ordinal differences only.  The lag-domain gradient contraction, the
 * predictive rank tables and the Toeplitz paths do not apply (lag_ok semantics unchanged).  agp_get_compact_stats: W, W n, and the
 * number of sweeps that read compact tables. */
int agp_get_lattice_stats(agp_ctx* ctx, int32_t* kind, int64_t* n_lattice, double* spacing);
int agp_get_compact_stats(agp_ctx* ctx, int32_t* lags_per_ordinal, int64_t* table_entries, int64_t* n_sweeps);
int agp_set_lattice(agp_ctx* ctx, int32_t on);
/* NaN-poison mode (env AGP_POISON=1 at agp_init; per context; a checking switch, not a path: results are bit for bit those of a
 * context without it).  Every fresh device allocation of floating-point values, every such workspace buffer when a call claims
 * it and the factor-store rows an extension sweep recomputes are filled with byte 0xFF (NaN), so a kernel that reads memory its
 * call has not written produces a NaN instead of a stale finite number.  Buffers holding addresses, indices, counts, times or
 * flags are never poisoned.  bytes / fills: what has been poisoned so far on this context (0 / 0 when the mode is off). */
int agp_get_poison_stats(agp_ctx* ctx, int64_t* bytes, int64_t* fills);
/* The admission test alone, on n time points in any order (host code only: no context, no device): kind as above, the lattice's
 * length and spacing, and per point its lattice index (index_out, nullable; -1 when kind = 0). */
int agp_probe_lattice(const double* ts, int64_t n, int32_t* kind, int64_t* n_lattice, double* spacing, int64_t* index_out);
/* One kernel program as a table-driven sweep compiles it (host code only: no context, no device): every maximal stationary subtree
 * with a transcendental leaf collapses into one table leaf, and the children of every binary node are ordered by the stack need of
 * the COMPILED tree (+ and x commute exactly, ChangePoint has a swapped form: no bit of the result depends on the order).
 * n_compiled: nodes of the compiled postfix program; chain: 1 when it has the form leaf (leaf binop)* — every binary node has a
 * leaf as one operand, so evaluating it needs no stack (one-node programs included); depth: its evaluation stack need; n_tables: its
 * table leaves.  All outputs nullable.  AGP_ERR_PROGRAM for a malformed program. */
int agp_probe_program(const uint8_t* ops, int32_t n_ops, const double* prm, int32_t n_prm, int32_t* n_compiled, int32_t* chain,
                      int32_t* depth, int32_t* n_tables);
/* How the particles of the last batch sweep (agp_logpdf_batch and its siblings, after deduplication) got their covariance tiles:
 * out5 = {evaluated inside the factorisation kernels as one-node programs, ... as chains in place (none yet: multi-node programs go
 * through the stack interpreter), ... by the stack interpreter, prebuilt by the tile builder, and of those prebuilt the multi-node
 * chains (the builder evaluates them without a stack)}. */
int agp_get_eval_stats(agp_ctx* ctx, int64_t* out5);

/* Reference arithmetic (AGP_REFERENCE_ARITHMETIC=1 at agp_init, or agp_set_reference_arithmetic(ctx, 1) right after it, before
 * agp_set_data).  The default engine picks, per call, among evaluators (direct, lag / rank tables), schedules (per-column,
 * dataflow, right-looking), structured sweeps (Toeplitz class), gradient contractions (lag domain, element-wise) and whatever the
 * factor store holds: all within the stated tolerances of one another, but a particle's low-order bits then depend on the batch it
 * travels in and on the order of the calls.  This switch selects ONE arithmetic whatever the state: every covariance element from
 * its own t_i - t_j (GammaExp by pow, src/GP.jl:285-289), tiles prebuilt, the left-looking Cholesky on one fixed schedule, the
 * dense joint predictive pass (V = L^-1 K12 for every query point, src/GP.jl:743-757), L^-T + K^-1 + the element-wise contraction
 * for every gradient, nothing resident (agp_logpdf_batch_extend = agp_logpdf_batch).  Results are then bit-identical across batch
 * sizes, call orders and single / batched / coalesced entries (tests/test_gpu_parity.py::test_reference_arithmetic_is_call_order_stable).
 * It overrides AGP_LAG / AGP_LAG_RANK / AGP_LATTICE / AGP_GRAD_LAGDOM / AGP_GRAD_FFT / AGP_FLOW / AGP_RIGHT_LOOKING /
 * AGP_SPLIT_DIAG / AGP_FUSE / AGP_GE_TABLE / AGP_FACTOR_CACHE / AGP_PREDICT_REUSE and cannot be switched off on a live context:
 * afterwards agp_set_lag_tables / agp_set_lag_rank_tables / agp_set_lattice / agp_set_grad_lag_domain / agp_set_factor_cache
 * return AGP_ERR_ARG for any non-zero argument, and agp_logpdf_batch_extend_multi runs plain sweeps like agp_logpdf_batch_extend. */
int agp_set_reference_arithmetic(agp_ctx* ctx, int32_t on);

/* OPT-IN structured value sweep (AGP_LAG=2 / agp_set_lag_tables(ctx, 2); off by default: the default path mirrors the reference's
 * dense Cholesky, src/Model.jl:134-136).  On the sorted copy of a regular grid a kernel that is a sum of stationary subtrees and
 * Linear leaves gives K = T + U C U' — T symmetric Toeplitz, U = [1, t], C 2x2 — and log N(x; 0, K) follows from log|T| and
 * L^-1 [x, 1, t] (T = L L') by the matrix determinant lemma and Woodbury's identity.  The Schur algorithm generates L column by
 * column from the generators of T's displacement (a hyperbolic rotation and a shift per column) without ever storing it: O(n^2)
 * flops per particle instead of n^3/3, stable for positive definite T.  Applies to agp_logpdf_batch with host outputs over n
 * CONSECUTIVE grid points of a series of n_max <= 4096 points: the whole series in any order, or a prefix of a series held in time
 * order (scripts/online.jl; fit_smc!(shuffle = false)) — a prefix of a shuffled grid is not; the other particles of the call, and any particle the structured sweep refuses (a reflection
 * coefficient of modulus >= 1: not positive definite to rounding), take the dense path, which also supplies LAPACK's info.
 * Taken when the class's share of the dense sweep would cost more than the recursion's n sequential steps (level 3 / AGP_LAG=3:
 * always).  Agreement with the dense path: <= 1e-10 of |logpdf| (tests/test_gpu_lag.py) for noises the reference can produce
 * (>= JITTER = 1e-5, src/Model.jl:22,134: <= 1e-9 in randomised runs with noises down to 1e-5); the Schur recursion is weakly stable —
 * on matrices with conditioning beyond 1e12 (noise 1e-12) where the dense factorisation itself keeps only 2-3 digits it keeps one
 * fewer.  agp_get_toeplitz_stats counts the particles scored that way.
 * The same level also makes the COALESCED single-particle entries class-aware (what Gen drives: every leapfrog step of Gen.hmc is
 * `update`, a value call, then `choice_gradients` at the same parameters, src/inference_smc_anneal_data.jl:63-67).  A coalesced
 * batch of agp_logpdf calls over the whole series scores its Toeplitz-class particles by the recursion and keeps them OUT of the
 * factor store; the others go through the store as before.  The agp_logpdf_grad batch that follows differentiates the class
 * particles that are not resident by the structured gradient sweep (Schur recursion + backward substitution, no dense factor) and
 * the others from their resident factors: per leapfrog no particle is factored twice, and the class never densely.  Both calls
 * apply the same size test (the class's share of the dense work against the two sequential passes of the structured gradient),
 * so a class too small to pay stays on the dense + store route in both.  Measured (tools/native/hmc_replay, n = 2048, regular
 * grid): 512 threads 402 -> 535 HMC iterations/s, 192 threads 343 -> 402, 64 / 128 threads unchanged (class below the size test). */
int agp_get_toeplitz_stats(agp_ctx* ctx, int64_t* n_particles);

/* Every OTHER sweep of agp_logpdf_batch{,_device,_multi} / agp_logpdf_grad_batch over (a prefix of) a regular grid of up to 4096
 * points — the annealing prefixes n < n_max of src/inference_smc_anneal_data.jl:206-217, the factorisation of a gradient sweep —
 * keeps the caller's order and reads the same stationary subtrees from RANK tables: |t_a - t_b| = |rank_a - rank_b| h whatever
 * the order of the points, so one table of n_max lags per subtree and sweep (instead of 255 per tile) serves every element.
 * Same agreement with the general path as the sorted sweeps.  AGP_LAG_RANK=0 / agp_set_lag_rank_tables(ctx, 0) disable it
 * (takes effect at the next sweep); agp_get_lag_rank_stats counts the sweeps of agp_logpdf_batch / agp_logpdf_grad_batch that used
 * it.  The factor store's sweeps (agp_logpdf_batch_extend, the coalesced batches of agp_logpdf) read rank tables too (the choice depends on the resident series alone, so an extension and a from-scratch sweep of
 * one entry still agree bit for bit — agp_set_data drops the store when an append changes the mode or the old points' ranks). */
int agp_set_lag_rank_tables(agp_ctx* ctx, int32_t on);
int agp_get_lag_rank_stats(agp_ctx* ctx, int64_t* n_sweeps);

/* Predictive passes whose query points sit on the series' own lattice — in every use of the reference the query set is
 * `train + test + future` at the data's cadence (scripts/online.jl:41-43; src/GP.jl:743 evaluates the kernel on [ts; ts_pred]):
 * every joint point then has an integer rank round((t - t_0) / h) (duplicates of training times share one, future points exceed
 * n_max - 1, earlier ones are negative), and agp_predict_batch reads the stationary subtrees from rank tables of max rank -
 * min rank + 1 <= 4096 lags, as the factor store's sweeps do.  One query point off the lattice (agp_set_data's tolerance) and
 * the call takes the general path.  No switch of its own (AGP_LAG=0 / AGP_LAG_RANK=0 cover it); agp_get_lag_predict_stats counts
 * the calls that took it. */
int agp_get_lag_predict_stats(agp_ctx* ctx, int64_t* n_passes);
/* ... and where, in addition, the n training points are consecutive grid points (256 <= n <= 2048), every query point is one of them
 * or a grid point after them (n + future points <= 4096), no covariance is requested and either nothing is resident in the
 * factor store or n >= 768 (from there on the two sequential passes of the recursion are cheaper than starting from resident
 * factors), the particles whose kernel is a sum of stationary subtrees and Linear leaves (at least 32 of them) need no dense
 * factor: one Schur recursion over the JOINT grid leaves L21 L11^-1 [x, 1, t] and the diagonal of T22 - T21 T11^-1 T12 per future
 * point, a backward substitution T11^-1 [x, e_first, 1, t]; predictions at training points come from alpha and diag(K11^-1)
 * (Gohberg-Semencul), the Linear leaves enter as a Bayesian linear model in [1, t] (Woodbury, update direction).  The other
 * particles of the call take the dense path; same results to ~1e-10 of their scale (tests/test_gpu_lag.py).  Part of AGP_GRAD_FFT >= 3
 * ("no dense factor where the structure allows"); agp_get_predict_structured_stats counts the particles served that way. */
int agp_get_predict_structured_stats(agp_ctx* ctx, int64_t* n_particles);

/* Gradient sweeps on a regular time grid (the points in any order, any prefix n <= n_max <= 4096): for a stationary kernel
 * dK_ab/dtheta depends on the lag |rank_a - rank_b| alone, so sum_ab G_ab dK_ab/dtheta = sum_g D_g dk(g h)/dtheta with D_g the
 * sum of G = 1/2 (alpha alpha' - K^-1) along the lag-g diagonals of the sorted series.  Particles whose kernel is a sum of
 * stationary subtrees (SquaredExponential, GammaExponential, Periodic, Constant, WhiteNoise under + and x) and Linear leaves
 * are contracted that way: the K^-1 tile kernel bins G by lag instead of writing the tile, and the reverse-mode pass of
 * Gen.choice_gradients' replacement (src/inference_smc_anneal_data.jl:63-67) runs over n lags instead of n^2 elements
 * (Linear leaves: three moments of G).  Same result as the element-wise contraction to rounding.
 * Linear leaves INSIDE products (no ChangePoint; at most d <= 3 of them along any product path; (2d+1) n_max <= 16376): at a
 * fixed lag the kernel is a polynomial of degree 2d in the pair's midpoint m = (t_a + t_b)/2, so the sum over the pairs at that
 * lag equals a sum over 2d+1 probe midpoints with moment-matched weights: the K^-1 tile kernel bins G m^k (k = 0..2d) by lag and
 * the reverse-mode pass runs over (2d+1) n virtual elements.  on = 2 (default; AGP_GRAD_LAGDOM=2) includes this class, 1 leaves it
 * to the element-wise contraction, 0 (AGP_GRAD_LAGDOM=0) disables the lag domain; the stats call counts the particles
 * contracted in the lag domain so far.
 *
 * Source of the lag sums of K^-1 (AGP_GRAD_FFT, default 3):
 *   0  histograms of the K^-1 tiles (any n_max <= 4096);
 *   1  power spectrum of the columns of L^-T (n_max <= 2048, n > 1024): no K^-1 tiles;
 *   2  where the sweep's n points are n CONSECUTIVE grid points — the whole series, or a prefix of a series given in time
 *      order, as data annealing adds it (src/inference_smc_anneal_data.jl:206-217) — and 256 <= n, n_max <= 2048:
 *      K = Toeplitz + the Linear leaves' rank-2 term in sorted order, and the lag sums follow from four solves with the
 *      Cholesky factor (right-hand sides x, e_first, 1, t) by the Gohberg-Semencul formula and a 2x2 Woodbury correction:
 *      O(n^2) per particle, no L^-T and no K^-1 at all.  Elsewhere as 1.  agp_get_grad_toeplitz_stats counts those particles.
 *   3  (default) as 2, and where no factor of the call's particles can be resident (empty factor store) and the class is large
 *      enough to pay for two sequential passes over n points, its particles skip the dense factorisation too: the Schur recursion
 *      on T (value, columns of L, forward substitution), a backward substitution, then the same lag-domain contraction with
 *      K^-1 = T^-1 - W S W' formed in the update direction (no downdate).  The value such a sweep reports agrees with the dense
 *      sweep's to ~1e-11 of |logpdf| (not bit for bit).  4 forces it whatever the class's size.
 *      agp_get_grad_structured_stats counts those particles. */
int agp_set_grad_lag_domain(agp_ctx* ctx, int32_t on);
int agp_get_grad_lag_domain_stats(agp_ctx* ctx, int64_t* n_particles);
int agp_get_grad_toeplitz_stats(agp_ctx* ctx, int64_t* n_particles);
int agp_get_grad_structured_stats(agp_ctx* ctx, int64_t* n_particles);

/* Value AND gradient: d logpdf / d theta for every (transformed) kernel parameter — out_grad has the
 * layout of `prm` (prm_off offsets; ChangePoint contributes d/dlocation, d/dscale) — and d logpdf / d noise.
 * This is what Gen.choice_gradients needs from the model body for Gen.hmc / Gen.map_optimize
 * (src/inference_smc_anneal_data.jl:63-67, src/Greedy.jl:95,370); the chain rule through
 * transform_param (src/Model.jl:24-48) stays on the host.  Kernel trees of up to 64 nodes. */
int agp_logpdf_grad_batch(agp_ctx* ctx, int64_t n, int32_t P,
                          const int32_t* op_off, const uint8_t* ops,
                          const int32_t* prm_off, const double* prm,
                          const double* noise,
                          double* out_logpdf /* P */, double* out_grad /* prm_off[P] */,
                          double* out_grad_noise /* P */, int32_t* out_info /* P */);

/* The same for ONE particle, for callers that differentiate one trace per thread (Gen.choice_gradients inside
 * Gen.hmc / Gen.map_optimize, one particle per Julia thread): re-entrant, concurrent callers are coalesced into
 * batched gradient sweeps exactly like agp_logpdf.  out_grad has n_prm entries (may be null when n_prm == 0). */
int agp_logpdf_grad(agp_ctx* ctx, int64_t n,
                    const uint8_t* ops, int32_t n_ops, const double* prm, int32_t n_prm,
                    double noise, double* out_logpdf, double* out_grad /* n_prm */,
                    double* out_grad_noise, int32_t* out_info);

/* Same sweep, results left in DEVICE memory (d_out_logpdf: P doubles, d_out_info: P int32,
 * both device pointers) and enqueued on `hip_stream` (a hipStream_t; NULL = the slot's own
 * stream, synchronised before return).  With a caller stream the call RETURNS AS SOON AS THE WORK IS ENQUEUED
 * (no host wait; the workspace stays reserved behind an event), so the caller chains its consumer — the
 * log-weight all-gather, agp_allgather_logweights_device — on the same stream and synchronises once.  This is the
 * entry the multi-GPU driver uses (src/inference_smc_anneal_data.jl:22-31,232 consume the gathered vector). */
int agp_logpdf_batch_device(agp_ctx* ctx, int64_t n, int32_t P,
                            const int32_t* op_off, const uint8_t* ops,
                            const int32_t* prm_off, const double* prm,
                            const double* noise,
                            double* d_out_logpdf, int32_t* d_out_info, void* hip_stream);
/* CONTRACT of the caller-stream form (changed in round 2, stated here once more because it is easy to miss): the
 * outputs are NOT complete when the call returns — read them only after synchronising hip_stream (or after work
 * ordered behind it on that stream).  Numerical failures are in d_out_info as usual.  The one failure that is not
 * numerical — a kernel's bounded wait for a diagonal factor giving up (info word -7; never observed, it exists so a
 * fault cannot hang the device) — cannot be returned by a call that does not wait: it is latched in the context when
 * the call's workspace is next claimed and fails the NEXT agp_logpdf_batch_device call, or agp_wait, with AGP_ERR_HIP.
 * agp_wait blocks until every asynchronously enqueued sweep of the context has completed and reports (and clears) that
 * latch; call it before trusting a run that never synchronises through another entry. */
int agp_wait(agp_ctx* ctx);

/* Posterior predictive of src/GP.jl:731-758 for P particles on the resident (ts, xs)[1:n].
 * mean_train (n) / mean_pred (m) are the values of the `mean` function (NULL = 0).
 * noise_pred may be NULL (= noise, src/GP.jl:739).  out_mean, out_var: m x P column-major;
 * out_cov: m x m x P (each slice symmetric) or NULL.  out_var = diag(out_cov) — the only part
 * Distributions.quantile consumes (src/GP.jl:1006-1012).  Identical particles (a resampled population) are evaluated
 * once (AGP_DEDUP=0 disables). */
int agp_predict_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                      const int32_t* op_off, const uint8_t* ops,
                      const int32_t* prm_off, const double* prm,
                      const double* noise, const double* noise_pred,
                      const double* mean_train, const double* mean_pred,
                      double* out_mean, double* out_var, double* out_cov,
                      int32_t* out_info);

/* Predictive log-density of held-out values (src/api.jl:686-699 predict_proba, test/experiment_hmc.jl:125):
 * out_logpdf[p] = logpdf(MvNormal(node_p, noise[p], ts[1:n], xs[1:n], ts_pred; noise_pred, mean), y_pred) for P particles on the
 * resident (ts, xs)[1:n] — the predictive of agp_predict_batch, scored without forming its covariance.  The joint matrix of the
 * training and query points is factored through all its block columns with noise_pred on the query diagonal; the query block's
 * log-det and Mahalanobis partials are the result.  noise_pred may be NULL (= noise); mean_train (n) / mean_pred (m) NULL = 0.
 * m == 0: logpdf 0 (the reference scores [] as 0); n == 0: the prior predictive N(y_pred; mean_pred, K22 + noise_pred I).
 * out_info[p] (may be NULL): 0; 1..n: K11 is not positive definite (first failing minor); n + k: K11 is, leading minor k of the
 * predictive covariance is not.  out_logpdf[p] is NaN whenever out_info[p] != 0; no particle affects another.  Identical particles
 * are evaluated once (AGP_DEDUP=0 disables).  Errors (negative return): m, n or P < 0, n > the uploaded series, a NULL input. */
int agp_predict_logpdf_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, const double* y_pred, int64_t m, int32_t P,
                             const int32_t* op_off, const uint8_t* ops,
                             const int32_t* prm_off, const double* prm,
                             const double* noise, const double* noise_pred,
                             const double* mean_train, const double* mean_pred,
                             double* out_logpdf, int32_t* out_info);

/* Quantiles of a Gaussian mixture, per point: Statistics.quantile(::MixtureModel, q; tol, max_iter) (src/api.jl:559-596) applied to
 * the mixture over components p of Normal(means[p*m + i], sqrt(vars[p*m + i])) with weights[p], at every point i < m and every
 * q[k], k < nq.  means / vars are column-major m x P (particle p's m values contiguous: the layout agp_predict_batch writes
 * out_mean / out_var in).  out_x[k*m + i]: the search's x; out_converged[k*m + i] (may be NULL): 1 if |cdf(x) - q| < tol held
 * within max_iter checks (the reference's `success` is the AND over all points); out_iters[k*m + i] (may be NULL, saturates at
 * INT32_MAX): the updates applied to x.  The reference's vectorised loop is reproduced bit for bit: start at 0 with
 * (x_min, x_max) = (-Inf, Inf), double until bracketed, then bisect; a point stops when it converges, at max_iter, when an
 * update leaves x unchanged (every later iteration would repeat it: the x of max_iter iterations, not converged), or — tol <= 0 —
 * once a cycle of its state is found, after the updates that take it to where max_iter would end.
 * cdf = sum over w_p != 0 of w_p normcdf((x - mu_p) / sigma_p), normcdf(z) = erfc(-z / sqrt 2) / 2; sigma_p == 0 is a step (0 below
 * mu_p, 1 above, 1/2 at x == mu_p).  A point's result depends only on its P components (in their order), q, tol and max_iter.
 * tol <= 0 and max_iter <= 0 are accepted (max_iter <= 0: x = 0, not converged).  m == 0 or nq == 0: nothing written.
 * Errors (negative return): P < 1; m, nq < 0; a q outside (0, 1) or NaN; weights not finite, negative or not summing to 1 (rtol
 * sqrt(eps)); at a positive weight, a non-finite mean or a negative or NaN variance; a NULL input; m*P or m*nq >= 2^31. */
int agp_mixture_quantile(agp_ctx* ctx, int64_t m, int32_t P, const double* means, const double* vars, const double* weights,
                         const double* q, int64_t nq, double tol, int64_t max_iter, double* out_x, int32_t* out_converged,
                         int32_t* out_iters);

/* predict_quantile(model, ds, q; noise_pred, tol, max_iter) (src/api.jl:547-557) on the resident (ts, xs)[1:n]: the marginal pass of
 * agp_predict_batch (out_cov = NULL; arguments n .. mean_pred as there), then predict_mvn's raw-space transform (src/api.jl:513-520)
 * of a linear y_transform, mu_raw = (mu - y_intercept) / y_slope and var_raw = (1 / y_slope^2) * var, then agp_mixture_quantile
 * with `weights` (the particle weights, P).  The m x P means and variances are staged through host memory between the two passes.
 * out_info[p] (may be NULL): 0; 1..n: K11 is not positive definite (agp_predict_batch's info); n + j: the raw marginal variance at
 * query j (1-based) is negative or NaN, or the raw mean there is not finite.  If any particle's info != 0, out_x is NaN everywhere
 * and nothing is converged (the reference throws).  Deviation: the reference builds MvNormal(mu, cov) from every particle's full
 * m x m predictive covariance, which throws PosDefException when that matrix is singular (e.g. duplicate query points with
 * noise_pred = 0); this entry, like predict_marginal, never forms it and so does not raise that error.  Errors as
 * agp_mixture_quantile (y_slope must be finite and non-zero, y_intercept finite) plus agp_predict_batch's. */
int agp_predict_quantile_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                               const int32_t* op_off, const uint8_t* ops,
                               const int32_t* prm_off, const double* prm,
                               const double* noise, const double* noise_pred,
                               const double* mean_train, const double* mean_pred, const double* weights,
                               double y_slope, double y_intercept, const double* q, int64_t nq, double tol, int64_t max_iter,
                               double* out_x, int32_t* out_converged, int32_t* out_iters, int32_t* out_info);

/* Posterior predictive samples: rand(MixtureModel(MvNormal_p, weights), S) of predict_mvn (src/api.jl:497-522) on the resident
 * (ts, xs)[1:n] — rand(predict_mvn(model, ds; noise_pred), S).  Arguments n .. mean_pred as agp_predict_logpdf_batch (noise_pred NULL
 * = each particle's noise, mean_train / mean_pred NULL = 0; n == 0 samples the prior K22 + noise_pred I).  Sample s is the column
 * out_x[s*m .. s*m + m) (Julia's m x S result of rand(d, S)):
 *     x_s = (mu*_c - y_intercept) / y_slope + (L22_c z_s) / |y_slope|,      c = c_s,  L22_c = chol(Sigma*_c)
 * — MvNormal((mu - b) / a, Sigma / a^2) of predict_mvn's raw-space transform, whose Cholesky factor is L22 / |a|.  mu*_c = mu2 + L21 a
 * and L22_c come from the joint factor of agp_predict_logpdf_batch's pass (the query right-hand side 0); no covariance is formed.
 *   component c_s: component[s] when given (S entries, each in [0, P) at a positive weight); else the inverse CDF of the cumulative
 *     weights (particle order, fp64 sums) at the uniform u_s: the first p with u_s < cum[p]; the last particle of positive weight when
 *     rounding leaves u_s >= cum[P-1] (a weight-0 particle is never drawn).  out_component[s] (may be NULL) receives c_s.
 *   normals z_s: z[s*m + i] when z is given (m*S entries); else z[s, i] = ndtri(u) (AS 241, as agp_predict_sum_batch).
 *   uniforms: Philox4x64-10 (Random123's constants, numpy.random.Philox) under the key (seed, 0); a 64-bit output word w gives
 *     u = ((w >> 11) + 0.5) * 2^-53 in fp64 (the one word that rounds to 1 gives 1 - 2^-53).  u_s is word 0 of the block of counter
 *     (s, 0, 0, 0); the u of z[s, i] is word i % 4 of the block (i / 4, s, 1, 0).
 * The bits of x[:, s] depend only on seed, s and the inputs of its component (its program, parameters, noise, noise_pred, the data,
 * ts_pred, the means and the transform): not on S, P, the particle order, copies, the workspace chunking or the other samples.
 * The draws are not Julia's RNG stream: the distribution, and the algebra given (c, z), are the contract.
 * m == 0 or S == 0: nothing is written.  out_info[p] (may be NULL): 0; 1..n: K11 is not positive definite (first failing minor); n + k:
 * leading minor k of the predictive covariance is not (agp_predict_logpdf_batch's convention).  If any particle's info != 0, out_x is
 * NaN everywhere (the reference throws PosDefException building that particle's MvNormal).  Identical particles are factored once
 * (AGP_DEDUP=0 disables); a sample drawn to any copy reads the shared factor.  Errors (negative return): P < 1; n, m or S < 0;
 * n > the uploaded series; weights not finite, negative or not summing to 1 (rtol sqrt(eps)); y_slope not finite or 0, y_intercept not
 * finite; a given component outside [0, P) or at weight 0; m*S >= 2^31; a NULL input. */
int agp_predict_sample_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                             const int32_t* op_off, const uint8_t* ops,
                             const int32_t* prm_off, const double* prm,
                             const double* noise, const double* noise_pred,
                             const double* mean_train, const double* mean_pred, const double* weights,
                             double y_slope, double y_intercept,
                             int64_t S, uint64_t seed, const int32_t* component /* S or NULL */,
                             const double* z /* m*S or NULL */,
                             double* out_x /* m*S column-major */, int32_t* out_component /* S or NULL */,
                             int32_t* out_info /* P or NULL */);

/* Moments of a mixture, Distributions.mean / var / cov of MixtureModel(components, weights): components p of mean means[p*m + i] and
 * covariance covs[p*m*m + j*m + i] (P blocks of m x m, column-major, symmetric: the lower triangle is read), weights[p].  means / vars
 * are column-major m x P (agp_predict_batch's layout).  covs NULL: the marginal moments from vars[p*m + i] (out_cov must be NULL); covs
 * given: the variances are its diagonals and vars is not read (may be NULL).  With e_p the component means,
 *     out_mean = sum w_p e_p,   out_cov = sum w_p (C_p + (e_p - mean)(e_p - mean)') (m x m, exactly symmetric),   out_var = diag(out_cov)
 * (out_var and the diagonal of out_cov are the same bits).  space 0: normal components N(means, covs).  space 1:
 * MvLogNormal(N(means, covs)) components (the direct-space view of a model fitted on log y): e_i = exp(mu_i + C_ii / 2),
 * C_p,ij = e_i e_j expm1(C_ij) (Distributions' MvLogNormal; src/Transforms.jl:87-91 on the diagonal).  A component mean past the
 * range of a double is Inf, which is the reference's behaviour and no error: out_mean is then Inf at that point — NaN if it is the
 * pivot's mean that overflowed (Inf - Inf) — and out_var and that row and column of out_cov are NaN, as (e - mean)^2 is with
 * mean = Inf.  The sums run on the device about a pivot (the first component of positive weight), sequentially in particle
 * order, with no atomics: the bits do not depend on agp_set_workspace_limit.  A component of weight 0 contributes nothing, whatever
 * it holds.  m == 0 writes nothing.  Errors (negative return): P < 1; m < 0; space outside {0, 1}; weights not finite, negative or
 * not summing to 1 (rtol sqrt(eps)); covs NULL with out_cov given; a NULL input; m*P >= 2^31, or m*m >= 2^31 with out_cov. */
int agp_mixture_moments(agp_ctx* ctx, int64_t m, int32_t P, const double* means, const double* vars, const double* covs,
                        const double* weights, int32_t space,
                        double* out_mean /* m */, double* out_var /* m */, double* out_cov /* m*m or NULL */);

/* mean / var / cov of predict_mvn(model, ds; noise_pred) (src/api.jl:497-522) on the resident (ts, xs)[1:n]: the MixtureModel over the
 * particles' posterior predictives with `weights`, after predict_mvn's raw-space transform of a linear y_transform,
 * mu_raw = (mu - y_intercept) / y_slope and C_raw = (1 / y_slope^2) C, in `space` (agp_mixture_moments: 0 the mixture itself, 1 its
 * MixtureModel(MvLogNormal.(components), weights) re-wrap).  Arguments n .. mean_pred as agp_predict_quantile_batch (n == 0: the prior).
 *   out_cov == NULL (marginal pass): agp_predict_batch's marginal pass (structured, lattice, store-reuse, duplicate-query and dedup
 *     paths), its m x P means and variances staged through host memory, then agp_mixture_moments' reduction on the device.
 *   out_cov != NULL (covariance pass): agp_predict_batch's pass with a covariance request; each chunk's covariances are added into
 *     the m x m running sums on the device and never leave it, nor do the per-particle marginals: m*m + 2m doubles come back instead
 *     of P*m*m.  Identical particles are
 *     evaluated once and their weights added onto the first copy (AGP_DEDUP=0 disables; agp_get_dedup_stats counts them).
 * out_info[p] (may be NULL): agp_predict_batch's.  If any particle's info != 0 — a particle of weight 0 included — every output is NaN
 * (the reference throws building that particle's MvNormal).  m == 0 writes nothing.  With profiling on, agp_get_timing's out[14..15]
 * = { the pass without the accumulation ms, the accumulation kernels ms } (marginal pass: of the staged reduction only).
 * Errors as agp_mixture_moments (y_slope must be finite and non-zero, y_intercept finite) plus agp_predict_batch's. */
int agp_predict_mixture_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                              const int32_t* op_off, const uint8_t* ops,
                              const int32_t* prm_off, const double* prm,
                              const double* noise, const double* noise_pred,
                              const double* mean_train, const double* mean_pred, const double* weights,
                              double y_slope, double y_intercept, int32_t space,
                              double* out_mean /* m */, double* out_var /* m */, double* out_cov /* m*m or NULL: marginal pass */,
                              int32_t* out_info /* P or NULL */);

/* infer_gp_sum(nodes, noise, ts, xs, ts_pred; noise_pred) (src/GP.jl:904-993) on the resident (ts, xs)[1:n]:
 * posterior of Z = [F_1(T*); ...; F_M(T*); X(T*)] for the sum-of-GPs model.  The M component kernels are
 * given as CSR-packed postfix programs (op_off / prm_off have M+1 entries).  out_mean: (M+1)*p;
 * out_cov: ((M+1)*p)^2 column-major symmetric (may be NULL); latent block i is rows [i*p, (i+1)*p),
 * the observable block is the last p rows — the index ranges the reference returns as (F, X). */
int agp_infer_gp_sum(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t p, int32_t M,
                     const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                     double noise, double noise_pred, double* out_mean, double* out_cov, int32_t* out_info);

/* infer_gp_sum for every particle of a population (src/api.jl:978-1034 calls GP.infer_gp_sum once per particle on the
 * split_kernel_sop of its kernel): particle p's components are CSR entries [p*M, (p+1)*M) (op_off / prm_off have P*M+1 entries), M
 * common to all particles.  Outputs in the reference's index order (F_1 .. F_M, X), per particle: out_mean and out_var P*(M+1)*p,
 * out_cov P*((M+1)p)^2 column-major or NULL (the marginal pass).  noise_pred NULL = each particle's own noise (the reference's
 * default).  Per particle the numbers are agp_infer_gp_sum's — noise[p] on the training diagonal, JITTER 1e-8 on every query row,
 * noise_pred[p] on the observable (X) rows only — with the dataflow schedule whatever the batch (the per-column one with AGP_FLOW=0):
 * a particle's bits do not depend on the batch size, order, copies or workspace chunking.  Identical particles (composite program,
 * parameters, noise, noise_pred) run once and share the first copy's bits.  n == 0 is the prior.  out_info[p] (may be NULL): 0, or
 * 1..n: the training block is not positive definite; a particle with info != 0 gets NaN in its own outputs only.  p == 0 writes
 * nothing.  Errors (negative return; the message names the particle where there is one): P < 1, M outside 1..200, p < 0,
 * n > n_max, malformed offsets, an unknown opcode, a composite program over AGP_MAX_OPS nodes (split trees can grow: (l+p)*(l+p)
 * expands), a NULL input, an output of 2^31 elements or more. */
int agp_infer_gp_sum_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t p, int32_t P, int32_t M,
                           const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                           const double* noise, const double* noise_pred,
                           double* out_mean, double* out_var, double* out_cov, int32_t* out_info);

/* predict_sum's numbers (src/api.jl:898-936 on top of predict_mvn_sum, 978-1034): the marginal pass of agp_infer_gp_sum_batch (no
 * covariance), then on the device predict_mvn_sum's raw-space transform of a linear y_transform, mu_raw = (mu - b)/a with + b/a on
 * the F_1 rows (the intercept counted once) and var_raw = (1/a^2) var (a = y_slope, b = y_intercept), then
 * quantile(Normal(mu_raw, sqrt(var_raw)), q[k]) per row (src/GP.jl:1006-1012) = fma(sqrt(var_raw), ndtri(q[k]), mu_raw), ndtri by
 * AS 241 (csrc/agp_ndtri.hpp: parity with the reference's erfcinv to rounding).  out_mean P*(M+1)*p raw means; out_x
 * P*(M+1)*p*nq, row-major per particle ((row, k) at row*nq + k); nq == 0: out_x is not written and may be NULL.  out_info[p]: as
 * agp_infer_gp_sum_batch, or n + j: joint row j (1-based) has a raw variance that is negative or NaN or a raw mean that is not
 * finite (the particle's outputs are NaN).  Errors: agp_infer_gp_sum_batch's, a q outside (0, 1) or NaN, y_slope not finite or
 * zero, y_intercept not finite. */
int agp_predict_sum_batch(agp_ctx* ctx, int64_t n, const double* ts_pred, int64_t p, int32_t P, int32_t M,
                          const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                          const double* noise, const double* noise_pred, double y_slope, double y_intercept,
                          const double* q, int64_t nq, double* out_mean, double* out_x, int32_t* out_info);

/* compute_cov_matrix_vectorized(node, noise, ts) (src/GP.jl:666-668) on explicit ts:
 * out_K is n x n column-major (full symmetric).  Parity / debugging entry. */
int agp_cov_matrix(agp_ctx* ctx, const double* ts, int64_t n,
                   const uint8_t* ops, int32_t n_ops, const double* prm, int32_t n_prm,
                   double noise, double* out_K);

/* ---- multi-GPU: particle sharding + the log-weight all-gather (RCCL over xGMI) --------------------------------
 * Particles are independent units: rank r of R evaluates the block [lo, hi) = agp_shard_range(P, r, R) of the
 * population on its own GPU (ts / xs replicated by agp_set_data, matrices never leave the GPU).  The only exchange
 * is the all-gather of the P log-weights that ESS / resampling consume on every rank
 * (compute_particle_weights / effective_sample_size, src/inference_smc_anneal_data.jl:22-31; Gen.maybe_resample!
 * at :232).  librccl is loaded on first use (dlopen, soname librccl.so.1; env AGP_RCCL_LIB overrides): single-GPU
 * users never need it. */
#define AGP_COMM_ID_BYTES 128    /* == sizeof(ncclUniqueId) */

/* first P % R ranks hold one particle more; identical on every rank */
void agp_shard_range(int32_t P, int32_t rank, int32_t n_ranks, int32_t* lo, int32_t* hi);
/* Cost-aware, duplicate-aware alternative for sweeps whose per-particle cost is NOT uniform (host code only; every rank derives
 * the same plan from the same population): sweep = 0 dense value sweep (uniform: use agp_shard_range), 1 gradient sweep,
 * 2 marginal predictive pass with m_future query points beyond the training points, 3 opt-in structured value sweep;
 * lattice_kind = the resident series' kind as agp_get_lattice_stats / agp_probe_lattice report it: 0 irregular (every particle
 * dense-priced), 1 regular grid — the particles whose kernel is a sum of stationary subtrees and Linear leaves cost O(n^2) in
 * sweeps 1-3 WHERE THE ENGINE ADMITS the structured sweep (the engine's own size tests, applied to the class particles one rank
 * will hold: n <= 2048 and a class large enough for sweep 1, n + m_future <= 4096 and >= 32 class particles for sweep 2, ...;
 * refused classes are dense-priced) —, 2 lattice with gaps (calendar indices: the class keeps its dense factor, only its gradient
 * contraction runs over the lattice's lags); 3 (a longer lattice served by compact tables: only tile evaluation differs) is priced
 * like 0.  Copies of an earlier particle (resampled populations,
 * src/inference_smc_anneal_data.jl:198-204) cost nothing and follow their representative.  Longest-processing-time greedy over
 * the distinct particles.  owner_out[p] = rank of particle p; cost_out[p] (nullable) = its modelled cost in units of one dense
 * factorisation (n^3/3 flops); rank_cost_out[r] (nullable) = the ranks' totals.  A rank evaluates its particles in ascending
 * index order; the all-gathered log-weights are put back in population order with the same owner_out (autogp.jl_amd/dist.py:
 * plan_indices / allgather_planned; the Julia shim's equivalent is a scatter by owner).  agp_logpdf_grad_batch_multi and
 * agp_predict_batch_multi below split by this plan themselves. */
int agp_shard_plan(int64_t n, int32_t P, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                   const double* noise, int32_t sweep, int32_t lattice_kind, int64_t m_future, int32_t n_ranks,
                   int32_t* owner_out, double* cost_out, double* rank_cost_out);

/* One process (or thread) per GPU: rank 0 creates the id, hands the 128 bytes to the other ranks over any host
 * channel (MPI, a file, Julia's Distributed, torch.distributed), every rank then joins with its own context. */
int agp_comm_get_unique_id(void* out_id /* AGP_COMM_ID_BYTES */);
int agp_comm_init_rank(agp_ctx* ctx, const void* id, int32_t n_ranks, int32_t rank);
/* returns 1 when the context has a communicator, 0 otherwise; rank / n_ranks may be NULL */
int agp_comm_info(agp_ctx* ctx, int32_t* rank, int32_t* n_ranks);
/* the number of ranks RCCL itself reports for the context's communicator (ncclCommCount); 0 without a communicator.
 * What a launcher prints to show that the ranks really met (bench.py: config.rccl_ranks_seen). */
int agp_comm_count(agp_ctx* ctx, int32_t* out_n_ranks);

/* One host process driving n_dev GPUs (a single Julia process): n_dev contexts + one communicator over them
 * (ncclCommInitAll).  out[i] is the context of device_ids[i] and rank i; destroy each with agp_destroy. */
int agp_init_multi(agp_ctx** out /* n_dev */, const int32_t* device_ids, int32_t n_dev);
int agp_set_data_multi(agp_ctx* const* ctxs, int32_t n_dev, const double* ts, const double* xs, int64_t n_max);
/* agp_remove_data on every context */
int agp_remove_data_multi(agp_ctx* const* ctxs, int32_t n_dev, const int64_t* idx, int64_t k);

/* All-gather of the log-weight vector.  Host form: inout_lw has P entries, this rank's block [lo, hi) filled on
 * entry, all P filled on return (every rank calls it; n_ranks == 1 is a no-op).  Device form: d_local holds the
 * hi - lo values of this rank (e.g. the d_out_logpdf of agp_logpdf_batch_device), d_all receives all P; enqueued on
 * hip_stream (NULL = engine stream, synchronised before return).  Blocks of unequal length are handled inside. */
int agp_allgather_logweights(agp_ctx* ctx, double* inout_lw, int32_t P);
int agp_allgather_logweights_device(agp_ctx* ctx, const double* d_local, int32_t P, double* d_all, void* hip_stream);

/* agp_logpdf_batch over the contexts of agp_init_multi: shards the P particles by agp_shard_range, runs every
 * shard's sweep concurrently (device 0's on the calling thread, the others on one persistent host thread per context,
 * created at the first call and joined by agp_destroy), all-gathers the log-weights over RCCL in one group call
 * and returns the complete vector (every device also keeps it).  out_logpdf / out_info: P entries, caller order. */
int agp_logpdf_batch_multi(agp_ctx* const* ctxs, int32_t n_dev, int64_t n, int32_t P,
                           const int32_t* op_off, const uint8_t* ops,
                           const int32_t* prm_off, const double* prm,
                           const double* noise, double* out_logpdf /* P */, int32_t* out_info /* P */);
/* The same with resident factors (agp_logpdf_batch_extend per shard): the reweight step of data annealing / add_data!
 * (src/inference_smc_anneal_data.jl:206-217, src/api.jl:426-443) for one process driving the node.  Every device keeps
 * the factors of its own shard; a particle that lands on another device after resampling is factored from scratch there. */
int agp_logpdf_batch_extend_multi(agp_ctx* const* ctxs, int32_t n_dev, int64_t n, int32_t P,
                                  const int32_t* op_off, const uint8_t* ops,
                                  const int32_t* prm_off, const double* prm,
                                  const double* noise, double* out_logpdf /* P */, int32_t* out_info /* P */);

/* The sweeps that dominate a fit, for one process driving several contexts: the reference threads EVERY per-particle operation
 * over the particles — the gradients of HMC rejuvenation (Gen.choice_gradients under Gen.hmc,
 * src/inference_smc_anneal_data.jl:63-67,240-252) and predict / predict_mvn (src/api.jl:508,645).  agp_logpdf_grad_batch /
 * agp_predict_batch over a list of contexts: the population is split by agp_shard_plan (sweep 1 / 2, the resident series' lattice
 * kind, the engine's own admission tests; copies follow their representative), every context's share runs concurrently (context
 * 0's on the calling thread, the others on their persistent host threads) and the results come back in the CALLER's order and
 * layout (exactly agp_logpdf_grad_batch's / agp_predict_batch's).  No collective is involved — results go to the host, which owns
 * the traces — so the contexts need not come from agp_init_multi: any distinct contexts holding the same data will do (several
 * contexts of one device included).  out_owner (nullable, P): the plan that was used. */
int agp_logpdf_grad_batch_multi(agp_ctx* const* ctxs, int32_t n_dev, int64_t n, int32_t P,
                                const int32_t* op_off, const uint8_t* ops,
                                const int32_t* prm_off, const double* prm,
                                const double* noise,
                                double* out_logpdf /* P */, double* out_grad /* prm_off[P] */,
                                double* out_grad_noise /* P */, int32_t* out_info /* P */, int32_t* out_owner /* P or NULL */);
int agp_predict_batch_multi(agp_ctx* const* ctxs, int32_t n_dev, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                            const int32_t* op_off, const uint8_t* ops,
                            const int32_t* prm_off, const double* prm,
                            const double* noise, const double* noise_pred,
                            const double* mean_train, const double* mean_pred,
                            double* out_mean, double* out_var, double* out_cov,
                            int32_t* out_info, int32_t* out_owner /* P or NULL */);

/* ---- measurement / debugging hooks (not part of the reference surface) ---- */

/* Factor a caller-supplied dense SPD matrix (n x n column-major) with the device Cholesky;
 * out_L receives the lower factor (n x n column-major, upper part zero). */
int agp_debug_cholesky(agp_ctx* ctx, const double* K, int64_t n, double* out_L, int32_t* out_info);

/* Factor P caller-supplied matrices (K: P blocks of n x n) with ONE chosen schedule of the batched Cholesky and return what the
 * diagonal tiles produce.  The tiles are packed from K (prebuilt tiles: no covariance is evaluated), the forward-solve vector is
 * seeded with y (P x n; NULL: zeros) and the factorisation runs through the host functions the sweeps call:
 *   schedule  0  one mixed launch per block column (diagonal + sub-diagonal tiles)
 *             1  split: diagonal-tile launch + sub-diagonal launch per block column
 *             2  right-looking: diagonal tile, panel solve, update of every trailing tile, per block column
 *             3  hybrid: mixed launches, then one catch-up launch and right-looking columns (AGP_ERR_ARG when the rule finds no
 *                switch column for (P, nt = ceil(n / 128)): nt < 3, or P (nt - 1) >= 512)
 *             4  the dataflow schedule (one launch of persistent workgroups)
 *            -1  what agp_logpdf_batch takes for (P, nt) under the context's settings (AGP_FLOW, AGP_SPLIT_DIAG, ...)
 * A schedule is never replaced by another one.  K must be symmetric, every entry given: element (r, c) of a block is read at
 * K[c * n + r] for r >= c (the lower triangle of a column-major matrix = the upper triangle of a row-major one); the diagonal
 * 128 x 128 tiles are packed with both triangles, and which of the two a schedule's diagonal kernel reads is its own business.
 * out_L: P x n x n, the lower factors (column-major, zero above the diagonal); out_beta (P x n, nullable): L^-1 y;
 * out_partial (P x 2, nullable): log det K = 2 sum log L_ii and beta' beta, the block columns' partials added in
 * agp_logpdf_batch's order; out_info (P): LAPACK info per matrix (0, or the 1-based index of the first non-positive pivot, whose
 * outputs are then meaningless).  A failed matrix leaves the others' outputs untouched, bit for bit. */
int agp_debug_factor_batch(agp_ctx* ctx, const double* K /* P*n*n */, const double* y /* P*n or NULL */,
                           int64_t n, int32_t P, int32_t schedule,
                           double* out_L /* P*n*n, lower */, double* out_beta /* P*n or NULL */,
                           double* out_partial /* P*2: logdet, beta'beta; or NULL */, int32_t* out_info /* P */);

/* Factor P caller-supplied matrices of ONE size 1 <= n <= AGP_SERIES_MAX_N with the factorisation of agp_logpdf_series_batch's kernel:
 * a second instantiation of that kernel loads matrix p (K: P blocks of n x n, row-major; only the lower triangle r >= c at
 * K[r * n + c] is read) and y (P x n; NULL: zeros) into the LDS layout where the production instantiations evaluate the
 * covariance (rows and columns past n: identity), then runs the SAME statements — blocked Cholesky in LDS, forward solve with one
 * refinement step, log-det and quadratic form, first bad pivot — and hands back what they leave:
 * out_L (P x n x n row-major, exact zeros above the diagonal), out_alpha (P x n) = L^-1 y, out_partial (P x 2) = 2 sum log L_ii and
 * alpha'alpha, out_lp (P) = -(n log 2 pi + the two partials) / 2 (NaN where out_info != 0), out_info (P) LAPACK info per matrix.
 * AGP_ERR_ARG: n < 1, n > AGP_SERIES_MAX_N, P < 1 or P > 65536, any null pointer but y.  Borrows a workspace slot like
 * agp_logpdf_series_batch and reads or changes nothing else the context holds.  A failed matrix leaves the others untouched. */
int agp_debug_series_factor(agp_ctx* ctx, const double* K /* P*n*n */, const double* y /* P*n or NULL */, int64_t n, int32_t P,
                            double* out_L /* P*n*n */, double* out_alpha /* P*n */, double* out_partial /* P*2 */,
                            double* out_lp /* P */, int32_t* out_info /* P */);

/* Factor P caller-supplied matrices of ONE size 1 <= n <= AGP_LONG_SERIES_MAX_N with the factorisation of
 * agp_logpdf_long_series_batch's long kernel: a second instantiation of that kernel writes block (ib, j) of matrix p (K, y: as for
 * agp_debug_series_factor) into the block's slot of the workgroup's HBM workspace where the production instantiations write the
 * covariance they evaluate (rows and columns past n: identity), then runs the SAME statements — left-looking block columns on the
 * packed workspace, panel products with the explicit inverse of the diagonal block, forward solve carried from registers with one
 * refinement step per block, log-det and quadratic form, first bad pivot — and hands back what they leave, in the shapes of
 * agp_debug_series_factor: out_L, out_alpha, out_partial, out_lp (NaN where out_info != 0), out_info.
 * AGP_ERR_ARG: n < 1, n > AGP_LONG_SERIES_MAX_N, P < 1 or P > 256, any null pointer but y.  Borrows a workspace slot and reads or
 * changes nothing else the context holds.  A failed matrix leaves the others untouched. */
int agp_debug_long_series_factor(agp_ctx* ctx, const double* K /* P*n*n */, const double* y /* P*n or NULL */, int64_t n, int32_t P,
                                 double* out_L /* P*n*n */, double* out_alpha /* P*n */, double* out_partial /* P*2 */,
                                 double* out_lp /* P */, int32_t* out_info /* P */);

/* Run agp_remove_data's update of resident factors on P caller-supplied factors of ONE size 2 <= n <= 1024.  Factor p (L0: P blocks of
 * n x n, row-major; only the lower triangle r >= c at L0[r * n + c] is read) and its forward-solve vector (alpha0: P x n; NULL:
 * zeros) are packed into arrays of the factor store's layout (tiles with the identity padding of the dense packer, inverse blocks
 * and partials per tile column, info = 0, slot p = factor p), every partial and every inverse block of the OLD grid is seeded with
 * the sentinel -7.0, and the positions idx (ascending, distinct, as agp_remove_data takes them) go run after run through the host
 * function agp_remove_data calls for a chunk of slots: nothing of the update is restated.  With n' = n - k, nt' = ceil(n' / 128)
 * and np' = 128 nt', what the kernels leave comes back at the new size:
 *   out_L        P x np' x np' row-major, the PADDED factor as it lies in the tiles: both triangles of the diagonal tiles, rows and
 *                columns from n' on included; the tile columns right of a tile row's diagonal tile do not exist and read 0
 *   out_alpha    P x np'
 *   out_partial  P x nt' x 2: 2 sum log L'_ii and sum alpha'_i^2 per tile column (the sentinel where the update wrote none)
 *   out_winv     P x nt' x 8 x 256 (nullable): the inverses of the 16 x 16 pivot blocks, block b of tile column J column-major at
 *                [((p nt' + J) 8 + b) 256 + 16 col + row] (the sentinel where the update wrote none)
 *   out_info     P: 0, or the 1-based position of the first new diagonal entry that is not finite and positive
 * AGP_ERR_ARG: n < 2, n > 1024, k < 1, k >= n, P < 1, P n^2 > 2^24 (or more than 2^27 doubles of padded tiles), positions not
 * ascending or out of range, any null pointer but alpha0 and out_winv.  Borrows a workspace slot and reads or changes nothing
 * else the context holds: not the store, the series, agp_get_remove_stats or agp_set_remove_update. */
int agp_debug_remove_factor(agp_ctx* ctx, const double* L0 /* P*n*n */, const double* alpha0 /* P*n or NULL */, int64_t n, int32_t P,
                            const int64_t* idx, int64_t k, double* out_L /* P*np'*np' */, double* out_alpha /* P*np' */,
                            double* out_partial /* P*nt'*2 */, double* out_winv /* P*nt'*8*256 or NULL */, int32_t* out_info /* P */);

/* Run the structured (Schur / Toeplitz) sweeps' launcher on P caller-supplied first columns of ONE size.  mode 0: the value sweep
 * (1 <= n <= 4096), 1: the gradient sweep's recursion and backward substitution (n <= 2048), 2: the predictive sweep's (n <= 2048
 * training points followed by nj - n future points, n <= nj <= 4096); nj is 0 or n in modes 0 and 1.  With N = nj in mode 2 and n
 * otherwise, particle p's first column r[p * N + g] (g = 0 .. N-1, WITHOUT the noise) is written into a lag table of the rank
 * layout, and the entry builds the particle's program itself from leaves[p] (NULL: all 0):
 *   bit 0  a second table r2[p * N + g]: two OP_LAG leaves under OP_PLUS (the kernel adds the tables entry by entry)
 *   bit 1  a Constant leaf of value const_v[p]          bit 2  a WhiteNoise leaf of value wn_v[p]
 *   bits 3-4  the number (0 to 2) of Linear leaves, leaf q with (centre, bias, amplitude) = lin[(2 p + q) * 3 + 0 .. 2]
 * raw_particle >= 0: that particle's program also gets a leaf with opcode raw_op (three zero parameters) — a leaf the kernels
 * refuse; -1: none.  noise (P), one shared x (n), and rank0, grid_h, grid_mid, t_ref as the sweeps pass them: point j of the
 * sweep has t - t_ref = (rank0 + j - grid_mid) grid_h.  Every output buffer is filled with the sentinel -7 (out_info: -7) before
 * the launch, so what a kernel did not store still reads -7:
 *   out_lp, out_info (P)   the log density and 0, or NaN and 1 for a refused particle (|rho| >= 1, a leaf that is not the kernels')
 *   out_Lcols    modes 1, 2: P x (n (n + 1) / 2 + 16), column k of L at k n - k (k - 1) / 2 - k + j for rows j = k .. n-1; the 16
 *                doubles after every triangle are never written
 *   out_fwd      modes 1, 2: P x 4 x ldv, ldv = 128 ceil(n / 128): L^-1 [x, e_first, 1, t - t_ref]
 *   out_sol      modes 1, 2: P x 4 x ldv: T^-1 [x, e_first, 1, t - t_ref] (left at the sentinel for a refused particle)
 *   out_pacc     mode 2: P x 4 x pstride, pstride = max(128, 128 ceil((nj - n) / 128)): per future point L21 L11^-1 [x, 1, t - t_ref]
 *                and the diagonal of T22 - T21 T11^-1 T12
 * AGP_ERR_ARG: a size the launcher refuses (above), n and nj inconsistent, P < 1 or P > 4096, more than 2^26 doubles of packed
 * triangles, leaves outside the bits above or without their values, a raw opcode outside 0 .. 255, any null pointer among the
 * arrays the mode uses.  Borrows a workspace slot and reads or changes nothing else the context holds. */
int agp_debug_toeplitz(agp_ctx* ctx, int32_t mode, int64_t n, int64_t nj, int32_t P, const double* r /* P*N */,
                       const double* r2 /* P*N or NULL */, const int32_t* leaves /* P or NULL */, const double* const_v /* P or NULL */,
                       const double* wn_v /* P or NULL */, const double* lin /* P*2*3 or NULL */, const double* noise /* P */,
                       const double* x /* n */, int32_t rank0, double grid_h, double grid_mid, double t_ref, int32_t raw_particle,
                       int32_t raw_op, double* out_lp /* P */, int32_t* out_info /* P */, double* out_Lcols, double* out_fwd,
                       double* out_sol, double* out_pacc);

/* The covariance tiles of a sweep over the first n >= 1 points of the RESIDENT series (agp_set_data first), entry by entry, on
 * whichever table path that sweep takes.  P >= 1 programs and noises in agp_logpdf_batch's format (no deduplication).  The entry
 * runs, unchanged and in their order, the stages a sweep runs up to its covariance launch — the table plan, the batch compilation
 * with the sweep's options plus "never fuse" (every tile then comes from the tile builder, as under AGP_FUSE=0), the geometry, the
 * slot's buffers, the staged upload, the lag tables — and launches the tile builder with the arguments a sweep's chunk builds.
 * for_gradient != 0: the plan of a gradient sweep (a whole grid takes rank tables in the caller's order instead of the sorted copy);
 * allow_tables = 0: the general evaluator whatever the series.  No factorisation runs (a matrix that is not positive definite is
 * returned like any other); the factor store, the coalescer, the dedup and sweep counters and agp_get_*_stats are neither read nor
 * changed; a workspace slot is borrowed.  Tiles and tables are filled with the sentinel -7 before the launches:
 *   out_K      P x n_pad x n_pad row-major, n_pad = 128 ceil(n / 128): the padded LOWER tiles as they lie — both triangles of the
 *              diagonal tiles, the padding rows and columns (identity: 1 on the diagonal, 0 elsewhere) — and -7 at every position
 *              of a tile above the diagonal tiles, which no sweep stores.  NULL: a sizing call, only out_mode is written.
 *   out_order  n: the position in the caller's series of row i of the sweep (the identity unless the plan runs on the sorted copy)
 *   out_mode   8 + P words: [0] the table mode (0 general evaluator, 1 lag tables on the sorted copy, 2 rank tables, 3 compact tables
 *              whole, 4 compact tables by tile window on the sorted copy), [1] LDS units of 256 doubles per table, [2] doubles per table
 *              in global memory (rank / compact layouts), [3] the number T of lag tables of the batch, [4] doubles per table in
 *              out_tab, [5] doubles in out_rep, [6] 1 when GammaExponential leaves read the log|dt| table, [7] the evaluation-stack
 *              depth of the tile builder's instantiation (4 or 8), [8 + p] how particle p is decoded: 0 one node, 1 chain, 2 stack
 *   out_tab    (nullable) T x out_mode[4]: the lag tables as the table kernel left them.  Rank and compact layouts: out_mode[2]
 *              entries per table; sorted layout: ceil(n / 128) block lags x 256, entry d + 127 of block lag b at lag 128 b + d
 *              (entry 255 is never read by a tile)
 *   out_rep    (nullable) out_mode[5]: the "time" every table entry was evaluated at, relative to out_rep[0] — the array the table
 *              kernel reads: the sorted series (sorted layout), the lattice times (rank), the compact entries' lag x spacing
 * AGP_ERR_ARG: what agp_logpdf_batch refuses (null context, null program or noise pointers), n < 1, P < 1, more than 2^27 doubles of
 * tiles, a null out_mode, a null out_order beside out_K; AGP_ERR_NODATA: n exceeds the resident series; AGP_ERR_PROGRAM as
 * agp_logpdf_batch (with for_gradient: as agp_logpdf_grad_batch). */
int agp_debug_cov_sweep(agp_ctx* ctx, int64_t n, int32_t P, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off,
                        const double* prm, const double* noise, int32_t for_gradient, int32_t allow_tables,
                        double* out_K /* P*n_pad*n_pad or NULL */, int32_t* out_order /* n */, int32_t* out_mode /* 8+P */,
                        double* out_tab /* or NULL */, double* out_rep /* or NULL */);

/* Probe of the fp64 MFMA fragment layout: D = A(16x4) * B(4x16), row-major host arrays. */
int agp_debug_mfma_probe(agp_ctx* ctx, const double* A, const double* B, double* D);

/* Element-wise probe of the device math used by the covariance kernels (csrc/agp_math.hpp):
 * which = 0 exp, 1 sin^2, 2 log, 3 pow(x, g), 4 erfc (the device library's, as the mixture-quantile kernel calls it),
 * 5 sqrt (the mixture-quantile kernels' sigma), 6 exp through the 128-entry table (exp_t, read from a copy in LDS as the
 * covariance kernels do), 7 / 8 the sine / cosine of sincos_pi_f, 9 expm1 (the device library's, as the mixture-moment kernels
 * call it). */
int agp_debug_math(agp_ctx* ctx, int32_t which, const double* x, const double* g, double* y, int32_t n);

/* fp64 MFMA issue-rate microbenchmark (16 independent accumulators per wave, wg_per_cu
 * workgroups of 4 waves per CU): sustained TFLOP/s and the shader clock while it ran.
 * Bits 8.. of wg_per_cu select what the waves execute (tools/gpu_dp_share.py): 0 MFMAs only, 1 fp64 VALU FMAs only
 * (128 per iteration), 2 both in every wave, 3 waves 0-1 MFMAs / waves 2-3 FMAs, 4 / 5 whole workgroups take one role
 * each (by block-index parity / by halves of 256 blocks); the TFLOP/s figure always assumes 16 MFMAs per wave and iteration. */
int agp_debug_mfma_peak(agp_ctx* ctx, int32_t iters, int32_t wg_per_cu, double* out_tflops, double* out_ghz);

/* Test hook: the un-padding of unequal shards after the padded all-gather (`padded`: n_ranks blocks of ceil(P/n_ranks)). */
int agp_debug_compact_shards(agp_ctx* ctx, const double* padded, int32_t P, int32_t n_ranks, double* out /* P */);

/* When enabled, batch calls bracket their phases with HIP events on the launch stream.
 * agp_get_timing fills out[0..7] = { total_ms, cov_build_ms, chol_update_ms, chol_trsm_ms,
 * finish_ms, n_update_launches, n_trsm_launches, h2d_d2h_ms } for the last batch call; a value+gradient sweep also
 * fills out[8..11] = { L^-T chain ms, K^-1 tiles ms, contraction ms, alpha + reductions ms }, agp_predict_sample_batch
 * out[12..13] = { normals ms, read-out ms }, agp_predict_mixture_batch out[14..15] = { pass ms, accumulation ms } (n_out up to 16).  The many-series entries fill
 * out[0] = out[2] = their fused kernels, and agp_predict_quantile_series_batch out[4] = its three read-out kernels,
 * agp_predict_logpdf_series_batch out[4] = its mixture read-out, agp_predict_sample_series_batch out[4] = its NaN-fill read-out. */
int agp_set_profiling(agp_ctx* ctx, int enabled);
int agp_get_timing(agp_ctx* ctx, double* out, int32_t n_out);
/* per-launch durations (ms) of the last profiled batch call: which = 0 update kernel, 1 trsm kernel;
 * returns the number of launches recorded (>= 0). */
int agp_get_launch_times(agp_ctx* ctx, int32_t which, double* out, int32_t n_out);

/* Coalescing of concurrent agp_logpdf callers: window in microseconds (0 = off) and counters. */
int agp_set_coalesce_window(agp_ctx* ctx, int32_t microseconds);
int agp_get_coalesce_stats(agp_ctx* ctx, int64_t* n_calls, int64_t* n_batches);
/* where the coalesced entries' wall time went since agp_init, microseconds: out4 = { leaders waiting for followers, value sweeps,
 * value + gradient sweeps (host side included), handing results back } */
int agp_get_coalesce_timing(agp_ctx* ctx, double* out4);

/* agp_logpdf_batch / agp_logpdf_grad_batch evaluate each distinct (program, parameters, noise) once and copy
 * the result to its duplicates (a resampled SMC population, src/inference_smc_anneal_data.jl:198-204, holds
 * many copies).  Counters: particles submitted / particles actually evaluated.  env AGP_DEDUP=0 disables. */
int agp_get_dedup_stats(agp_ctx* ctx, int64_t* n_particles, int64_t* n_evaluated);
/* Mixture-moment passes (agp_mixture_moments, agp_predict_mixture_batch) since agp_init: how many finished and how many chunks of
 * components their running sums took in (more chunks than passes: agp_set_workspace_limit split a pass). */
int agp_get_mixture_stats(agp_ctx* ctx, int64_t* n_passes, int64_t* n_chunks);

/* Cap (bytes) on matrix workspace per call; larger batches are processed in chunks. 0 = default. */
int agp_set_workspace_limit(agp_ctx* ctx, int64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* AUTOGP_HIP_H */
