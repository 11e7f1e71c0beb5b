// Host-side launch interface between the orchestration (agp_engine.hip) and the kernel translation units:
//   agp_kernels.hip         covariance evaluation + factorisation + the small service kernels
//   agp_kernels_grad.hip    gradient sweep (L^-T chains, K^-1 tiles, spectra, contractions)
//   agp_kernels_series.hip  small-matrix value kernel and its value-and-gradient twin (one workgroup per particle of a short series)
//   agp_kernels_long_series.hip  long-series value kernel (one workgroup per particle of a series of up to 512 points, factor in HBM)
//   agp_kernels_long_series_probe.hip  its probe instantiation (caller matrices; agp_debug_long_series_factor)
//   agp_kernels_long_series_predict.hip  its predictive twin (the posterior at the series' own query times behind the value)
//   agp_kernels_long_series_proba.hip  its held-out twin (the joint points factored, the query rows' partials read out)
// Every template instantiation lives behind one of these plain functions, so the units compile in parallel and the
// function attributes (dynamic-LDS ceilings) are set on the copies that are actually launched.
#pragma once
#include "agp_args.hpp"

namespace agp {

// ---- agp_kernels.hip -------------------------------------------------------------------------------------------------
hipError_t kernels_init();          // raises the dynamic-LDS ceiling of the table-carrying covariance kernels (once, agp_init)
// tile builder: ntiles lower tiles of particles [ca.p_off, ca.p_off + P) (LDS for max_cp per-point tables and the node records of
// programs of up to max_ops nodes, stack depth 4 / 8)
hipError_t launch_cov(hipStream_t st, const CovArgs& ca, int ntiles, int P, int max_cp, int depth, int max_ops);
void launch_lag_tables(hipStream_t st, const LagArgs& la, int units, int n_tables);
hipError_t launch_toep_logpdf(hipStream_t st, const ToepArgs& ta);      // structured value sweep: one workgroup per particle (ta.P)
void launch_logdt_tiles(hipStream_t st, unsigned ntiles, const double* ts, double* out);
// DCOV selection (dcov): 0 = tiles are resident, 4 / 8 = evaluate the kernel program in the kernel with that evaluation-stack
// depth; ca.lag / ca.logdt select the table-reading instantiations (GM 2 / 1, see chol_tile).
void launch_update_factor(int dcov, int grid, hipStream_t st, const CholArgs& ca);     // block column: diagonal + sub-diagonal tiles
void launch_update_subdiag(int dcov, int grid, hipStream_t st, const CholArgs& ca);    // sub-diagonal tiles only (dominant kernel)
void launch_update_schur(int dcov, int grid, hipStream_t st, const CholArgs& ca);      // Schur / catch-up pass (no factorisation)
void launch_diag(int dcov, int grid, hipStream_t st, const CholArgs& ca);              // diagonal tiles, one workgroup per particle
void launch_flow(int dcov, int n_wg, hipStream_t st, const CholArgs& ca);              // dataflow schedule, persistent workgroups
void launch_trsm(int grid, hipStream_t st, const CholArgs& ca);                        // panel solve of the right-looking schedule
void launch_init_vec(hipStream_t st, int ldv, int P, double* vec, const double* xs, const double* mu1, int n1, int* info, int* ready);
void launch_finish_logpdf(hipStream_t st, const double* partial, const int* info, int nt, int P, int n, const int* map,
                          double* out_logpdf, int* out_info, const int* slot = nullptr, int ntp = 0);
// predictive log-density (agp_predict_logpdf_batch): y* - mu2 into the query segment; the query columns' partials -> logpdf, info
void launch_init_query_vec(hipStream_t st, int P, double* vec, int ldv, int off, int m, const double* y, const double* mu2);
void launch_finish_pred_logpdf(hipStream_t st, const double* partial, const int* info, int nt1, int nt, int P, int m, int n,
                               int n1_pad, const int* map, double* out_logpdf, int* out_info);
void launch_init_extend(hipStream_t st, int U, double* vec, int ldv, int n_pad, const double* xs, int n, const int* slot,
                        const int* i0, int* info, int* ready);
void launch_init_flow_flags(hipStream_t st, int P, int* tflag, int ntri_stride, int ntri, const int* slot, const int* i0);
void launch_gather_factor(hipStream_t st, int gx, int P, const GatherArgs& ga);
void launch_copy_rows(hipStream_t st, int gx, int rows, double* dst, long long dpitch, const double* src, long long spitch, long long width);
void launch_poison_rows(hipStream_t st, int gx, int U, int nbuf, const PoisonRowsArgs& a);   // AGP_POISON: store rows a sweep recomputes -> NaN (nbuf <= 4)
void launch_scatter_uploads(hipStream_t st, const void* blob, int n_items, int slices);      // PinnedUploads: one blob -> its destinations
void launch_expand_rep(hipStream_t st, int P, const double* lp, const int32_t* rep, double* out);
void launch_pred_extract(hipStream_t st, long long nel, int P, const PredArgs& pa);
void launch_unpack_dense(hipStream_t st, const double* A, int n, int lower_only, double* out);
void launch_pack_dense(hipStream_t st, const double* K, int n, int nt, long long n_packed, double* A);
void launch_compact_shards(hipStream_t st, const double* padded, int mx, int P, int n_ranks, double* out);
void launch_mfma_probe(const double* A, const double* B, double* D);
void launch_math_probe(int which, const double* x, const double* g, double* y, int n);
void launch_mfma_peak(int nblk, double* out, long long* cycles, int iters, int mode);
// mixture quantiles (agp_quantile.hip): components to one row per point (sigma = sqrt(var)), then one wave per (point, q)
void launch_mixture_pack(hipStream_t st, const double* means, const double* vars, int P, int Pp, int m, double* cm, double* cs);
void launch_mixture_quantile(hipStream_t st, const double* cm, const double* cs, const double* cw, int Pp, int m, const double* q,
                             int nq, double tol, long long max_iter, double* out_x, int32_t* out_conv, int32_t* out_iters);
// agp_predict_quantile_series_batch's read-out (agp_series.hip; agp_series_quantile_kernel.hpp): pack (always: it also writes the info
// words), the searches (a.nq > 0) and the marginal moments (a.out_mean or a.out_var) of n_queries = q_off[S] query points;
// max_rows_el = the largest m_s Pp_s of a series
void launch_series_mix_readout(hipStream_t st, const SeriesQuantArgs& a, long long n_queries, long long max_rows_el);
// agp_predict_logpdf_series_batch's read-out: the log mixture density of every series' held-out vector, one thread per series
void launch_series_mix_logp(hipStream_t st, const SeriesMixLogpArgs& a);
// predict_sum's read-out (agp_predict.hip): raw transform, F_1 intercept, marginal quantiles on a chunk's device marginals
void launch_sum_readout(hipStream_t st, int P, const SumReadArgs& a);
// posterior predictive samples (agp_sample.hip): the normals of every sample column, then per chunk one workgroup per (group of
// SMP_G samples of one particle, query tile row)
void launch_philox_normals(hipStream_t st, const SampleNormArgs& a);
void launch_pred_sample(hipStream_t st, int n_groups, int nt2, const SampleReadArgs& a);
// mixture moments (agp_mixmom.hip): one chunk of components onto the running sums (a.cov null: S1 and the diagonal only), then the
// finish (a.out_cov null: the marginal one)
void launch_mixmom_chunk(hipStream_t st, const MixMomArgs& a);
void launch_mixmom_finish(hipStream_t st, const MixMomArgs& a);

// ---- agp_kernels_grad.hip --------------------------------------------------------------------------------------------
hipError_t kernels_init_grad();
void launch_trtri_chain(hipStream_t st, int grid, const GradArgs& ga);
void launch_zspec(hipStream_t st, int nt, int P, const GradArgs& ga);
void launch_toep_solve(hipStream_t st, int P, size_t lds, const GradArgs& ga);      // ga.plist: the particles, one workgroup each
void launch_kinv_tiles(hipStream_t st, int grid, const GradArgs& ga);
hipError_t launch_grad_contract(int maxs, hipStream_t st, const GradArgs& ga, int ntiles, int P, size_t lds);      // maxs: 64 / 16 / 0 (LDS tape)
void launch_lag_grad(hipStream_t st, int P, size_t lds, const GradArgs& ga);
void launch_grad_finish(hipStream_t st, int P, const GradArgs& ga);

// ---- agp_kernels_series.hip ------------------------------------------------------------------------------------------
hipError_t kernels_init_series();   // raises the dynamic-LDS ceiling of k_series_logpdf / k_series_logpdf_grad / k_series_predict / k_series_predict_logpdf / k_series_predict_sample / k_series_predict_sum to the whole 160 KiB (once, agp_init)
// small-matrix value kernel: one workgroup per entry of sa.wg (`grid` of them), evaluation-stack depth 4 / 8, lds_bytes = the largest
// SeriesLds total of the launch's particles
hipError_t launch_series_logpdf(hipStream_t st, const SeriesArgs& sa, int grid, int depth, size_t lds_bytes);
// value-and-gradient twin: tape = nodes of the reverse-mode tape (16 / 64); the evaluation-stack depth is the value kernel's for the same
// program (a tree of <= 16 nodes never needs more than 4), lds_bytes = the largest SeriesGradLds total of the launch's particles
hipError_t launch_series_logpdf_grad(hipStream_t st, const SeriesGradArgs& sa, int grid, int depth, int tape, size_t lds_bytes);
hipError_t kernels_init_series_hmc();   // ... and of k_series_hmc (agp_kernels_series_hmc.hip)
// HMC twin (k_series_hmc): the same rule; lds_bytes = the largest series_hmc_lds total of the launch's particles
hipError_t launch_series_hmc(hipStream_t st, const SeriesHmcArgs& sa, int grid, int depth, int tape, size_t lds_bytes);
// predictive twin (k_series_predict): depth as for the value kernel, lds_bytes = the largest series_pred_lds total of the launch's particles
hipError_t launch_series_predict(hipStream_t st, const SeriesPredArgs& sa, int grid, int depth, size_t lds_bytes);
// decomposition twin (k_series_predict_sum): as the predictive twin, on composite programs (their selector tables counted in lds_bytes)
hipError_t launch_series_predict_sum(hipStream_t st, const SeriesSumArgs& sa, int grid, int depth, size_t lds_bytes);
// held-out twin (k_series_predict_logpdf): depth as for the value kernel, lds_bytes = the largest series_lds total of the launch's
// particles at their JOINT lengths n_s + m_s
hipError_t launch_series_predict_logpdf(hipStream_t st, const SeriesProbaArgs& sa, int grid, int depth, size_t lds_bytes);
// sampling twin (k_series_predict_sample): as the held-out twin; k_series_sample_fill behind it, one workgroup per series
hipError_t launch_series_predict_sample(hipStream_t st, const SeriesSampleArgs& sa, int grid, int depth, size_t lds_bytes);
hipError_t launch_series_sample_fill(hipStream_t st, const SeriesSampleFillArgs& a);
// its probe instantiation on caller matrices: workgroup b factors matrix b of `grid`, lds_bytes = series_lds(sa.n, 0, 0, 0).total doubles
hipError_t launch_series_probe(hipStream_t st, const SeriesProbeArgs& sa, int grid, size_t lds_bytes);

// ---- agp_kernels_long_series.hip -------------------------------------------------------------------------------------
hipError_t kernels_init_long_series();   // raises the dynamic-LDS ceiling of k_long_series_logpdf to the whole 160 KiB (once, agp_init)
// long-series value kernel: one workgroup per entry of la.wg (`grid` of them), each with la.ws_stride doubles of la.ws for its factor;
// evaluation-stack depth 4 / 8, lds_bytes = the largest long_series_lds total of the launch's particles
hipError_t launch_long_series_logpdf(hipStream_t st, const LongSeriesArgs& la, int grid, int depth, size_t lds_bytes);

// ---- agp_kernels_long_series_predict.hip -----------------------------------------------------------------------------
hipError_t kernels_init_long_series_predict();   // the same ceiling for k_long_series_predict (once, agp_init)
// predictive twin: the launch above with the query side; lds_bytes = the largest long_series_pred_lds total of the launch's
// particles, la.ws_stride >= 256 long_series_pred_ws_blocks(nb) for each of them
hipError_t launch_long_series_predict(hipStream_t st, const LongSeriesPredArgs& la, int grid, int depth, size_t lds_bytes);

// ---- agp_kernels_long_series_proba.hip -------------------------------------------------------------------------------
hipError_t kernels_init_long_series_proba();   // the same ceiling for k_long_series_predict_logpdf (once, agp_init)
// held-out twin: the value launch on the JOINT points with the query side; lds_bytes = the largest long_series_lds total of the
// launch's particles at their joint lengths n_s + m_s, la.ws_stride >= 256 long_series_ws_blocks(nb) for each of them
hipError_t launch_long_series_predict_logpdf(hipStream_t st, const LongSeriesProbaArgs& la, int grid, int depth, size_t lds_bytes);

// ---- agp_kernels_long_series_probe.hip -------------------------------------------------------------------------------
// one workgroup per caller matrix: lds_bytes = long_series_lds(la.n, 0, 0, 0), la.ws_stride >= 256 nb (nb + 1) / 2
hipError_t launch_long_series_probe(hipStream_t st, const LongSeriesProbeArgs& la, int grid, size_t lds_bytes);

}  // namespace agp
