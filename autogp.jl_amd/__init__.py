"""MI355X-native GP marginal-likelihood engine for AutoGP.jl's hot path.

The directory name follows the repo convention (`autogp.jl_amd`); because of the dot it is
imported through `__graft_entry__.load_package()` (module name ``autogp_jl_amd``).
"""
from .gp import (Node, LeafNode, BinaryOpNode, WhiteNoise, Constant, Linear, SquaredExponential,
                 GammaExponential, Periodic, Plus, Times, ChangePoint, unroll, encode, encode_batch, from_tuple,
                 split_kernel_sop, extract_kernel)
from .engine import (GPEngine, GPEngineMulti, shard_range, shard_plan, probe_lattice, probe_program, logpdf_grad_batch_multi, predict_batch_multi, AGPError, PosDefException, load_library, LIB_PATH, EXPORTED_SYMBOLS,
                     compute_cov_matrix_vectorized, eval_cov, mvnormal_logpdf, MvNormal, quantile, infer_gp_sum, predict_proba,
                     predict_quantile, predict_quantile_multi, raw_components, predict_mvn_sum, predict_sum, predict_rand,
                     MixtureModel, predict_mvn, pack_series, series_call_args, pack_queries, SERIES_MAX_N, LONG_SERIES_MAX_N, LONG_SERIES_ALL,
                     pack_series_mixture, predict_quantile_series, SeriesBand, pack_heldout, predict_proba_series, SeriesScores,
                     predict_rand_series, predict_mvn_series, SeriesSamples, SeriesMixtureModel, predict_sum_series, SeriesSums,
                     mcmc_parameters_series, with_params)
from . import prior, schedule, dist, stream

__all__ = [n for n in dir() if not n.startswith("_")]
