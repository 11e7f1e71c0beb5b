// Host side of the mixture moments: Distributions.mean / var / cov of the MixtureModel that predict_mvn returns (src/api.jl:497-522),
// and of its MvLogNormal re-wrap (docs/src/tutorials/iclaims.md; Transforms.jl:87-91), on components the caller supplies
// (agp_mixture_moments) and on the resident series (agp_predict_mixture_batch).  The reduction over the particles runs on the device
// (csrc/agp_mixmom_kernel.hpp) with running sums that continue from chunk to chunk of the pass.
#include "agp_host.hpp"

// (profiling) a new pair of events, owned by mp.ev from its creation on, the first recorded on st
static hipError_t mix_mark(MixPass& mp, hipStream_t st) {
  mp.ev.push_back({nullptr, nullptr});
  if (const hipError_t e = hipEventCreate(&mp.ev.back().first)) return e;
  if (const hipError_t e = hipEventCreate(&mp.ev.back().second)) return e;
  return hipEventRecord(mp.ev.back().first, st);
}

int mix_stage(agp_ctx* c, Slot* s, hipStream_t st, PinnedUploads& up, MixPass& mp, int64_t m, const std::vector<double>& w_pass) {
  mp.m = m; mp.started = false;
  mp.w_pass = w_pass;
  const size_t P = w_pass.size();
  mp.q_first = (int)P;
  for (size_t q = 0; q < P; ++q) if (w_pass[q] > 0.0) { mp.q_first = (int)q; break; }
  HIPCHK(c, s->mix_w.ensure(sizeof(double) * std::max<size_t>(1, P)));
  HIPCHK(c, s->mix_s.ensure(sizeof(double) * 3 * (size_t)std::max<int64_t>(1, m)));
  HIPCHK(c, s->mix_out.ensure(sizeof(double) * ((size_t)2 * m + (mp.cov ? (size_t)m * m : 0) + 1)));
  if (mp.cov) HIPCHK(c, s->mix_acc.ensure(sizeof(double) * (size_t)std::max<int64_t>(1, m * m)));
  up.add(s->mix_w.p, mp.w_pass.data(), sizeof(double) * P);
  mp.profiling = c->profiling;      // (latched: agp_set_profiling during the pass changes nothing of it)
  if (mp.profiling) HIPCHK(c, mix_mark(mp, st));
  return AGP_OK;
}

namespace {

MixMomArgs mix_args(Slot* s, const MixPass& mp) {
  MixMomArgs a = {};
  const int64_t m = mp.m;
  a.m = (int)m; a.space = mp.space;
  a.slope = mp.slope; a.intercept = mp.intercept; a.ivar = 1.0 / (mp.slope * mp.slope);
  a.e = s->mix_e.as<double>();
  a.s = s->mix_s.as<double>(); a.s1 = a.s + m; a.s2d = a.s + 2 * m;
  a.acc = mp.cov ? s->mix_acc.as<double>() : nullptr;
  a.out_mean = s->mix_out.as<double>(); a.out_var = a.out_mean + m;
  a.out_cov = mp.cov ? a.out_mean + 2 * m : nullptr;
  return a;
}

}  // namespace

int mix_chunk(agp_ctx* c, Slot* s, hipStream_t st, MixPass& mp, int p0, int Pc, const double* d_mean, const double* d_var,
              const double* d_cov) {
  if (mp.m <= 0 || Pc <= 0 || p0 + Pc <= mp.q_first) return AGP_OK;      // (nothing of positive weight yet: the sums have not begun)
  HIPCHK(c, s->mix_e.ensure(sizeof(double) * (size_t)mp.m * Pc));
  MixMomArgs a = mix_args(s, mp);
  a.mean = d_mean; a.cov = d_cov;
  if (d_cov) { a.var = d_cov; a.v_pstride = (long long)mp.m * mp.m; a.v_istride = mp.m + 1; }
  else { a.var = d_var; a.v_pstride = mp.m; a.v_istride = 1; }
  a.w = s->mix_w.as<double>() + p0; a.Pc = Pc;
  a.pivot = mp.started ? -1 : mp.q_first - p0;
  mp.started = true;
  if (mp.profiling) HIPCHK(c, mix_mark(mp, st));
  launch_mixmom_chunk(st, a);
  HIPCHK(c, hipGetLastError());
  if (mp.profiling) HIPCHK(c, hipEventRecord(mp.ev.back().second, st));
  ++mp.n_chunks;
  return AGP_OK;
}

int mix_finish(agp_ctx* c, Slot* s, hipStream_t st, MixPass& mp) {
  const int64_t m = mp.m;
  if (m <= 0) return AGP_OK;
  if (!mp.started) return fail(c, AGP_ERR_ARG, "no component of positive weight");
  MixMomArgs a = mix_args(s, mp);
  launch_mixmom_finish(st, a);
  HIPCHK(c, hipGetLastError());
  if (mp.profiling) HIPCHK(c, hipEventRecord(mp.ev[0].second, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // (blocking copies: nothing in flight towards the caller's arrays on an error return)
  HIPCHK(c, hipMemcpy(mp.out_mean, a.out_mean, sizeof(double) * m, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(mp.out_var, a.out_var, sizeof(double) * m, hipMemcpyDeviceToHost));
  if (mp.cov) HIPCHK(c, hipMemcpy(mp.out_cov, a.out_cov, sizeof(double) * m * m, hipMemcpyDeviceToHost));
  {
    std::lock_guard<std::mutex> g(c->mu);
    ++c->n_mix_passes; c->n_mix_chunks += mp.n_chunks;
  }
  if (mp.profiling) {
    float total = 0.0f;
    double acc = 0.0;
    HIPCHK(c, hipEventElapsedTime(&total, mp.ev[0].first, mp.ev[0].second));
    for (size_t k = 1; k < mp.ev.size(); ++k) {
      float ms = 0.0f;
      HIPCHK(c, hipEventElapsedTime(&ms, mp.ev[k].first, mp.ev[k].second));
      acc += ms;
    }
    std::lock_guard<std::mutex> g(c->mu);
    c->timing[14] = (double)total - acc; c->timing[15] = acc;
  }
  return AGP_OK;
}

namespace {

int check_mixture(agp_ctx* c, int64_t m, int32_t P, const double* weights, int32_t space, bool want_cov) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (P <= 0) return fail(c, AGP_ERR_ARG, "P must be >= 1");
  if (m < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (space != 0 && space != 1) return fail(c, AGP_ERR_ARG, "space must be 0 (normal) or 1 (log-normal)");
  const int64_t Pp = ((int64_t)P + 63) / 64 * 64;
  if (m * Pp >= ((int64_t)1 << 31) || (want_cov && m * m >= ((int64_t)1 << 31))) return fail(c, AGP_ERR_ARG, "m * P or m * m too large");
  return check_weights(c, P, weights);
}

void fill_nan(MixPass& mp, int64_t m) {
  const double nanv = std::numeric_limits<double>::quiet_NaN();
  std::fill(mp.out_mean, mp.out_mean + m, nanv);
  std::fill(mp.out_var, mp.out_var + m, nanv);
  if (mp.cov) std::fill(mp.out_cov, mp.out_cov + m * m, nanv);
}

// components on the host (column-major m x P means / vars, P blocks of m x m covs or null) -> the moments, uploaded chunk by chunk
int mixture_core(agp_ctx* c, int64_t m, int32_t P, const double* means, const double* vars, const double* covs, const double* weights,
                 MixPass& mp) {
  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const int64_t bytes_pp = std::max<int64_t>(1, (covs ? m * m : 2 * m) * 8);
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(P, ws_limit_bytes(c) / bytes_pp));
  HIPCHK(c, s->pred_mean.ensure(sizeof(double) * (size_t)m * chunk));
  if (covs) HIPCHK(c, s->pred_cov.ensure(sizeof(double) * (size_t)m * m * chunk));
  else HIPCHK(c, s->pred_var.ensure(sizeof(double) * (size_t)m * chunk));
  PinnedUploads up;
  if (const int rc = mix_stage(c, s, st, up, mp, m, std::vector<double>(weights, weights + P))) return rc;
  HIPCHK(c, up.flush(s->h_stage, s->up_blob, st));
  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int Pc = std::min(chunk, P - p0);
    if (p0 + Pc <= mp.q_first) continue;
    HIPCHK(c, hipMemcpyAsync(s->pred_mean.p, means + (size_t)p0 * m, sizeof(double) * (size_t)m * Pc, hipMemcpyHostToDevice, st));
    if (covs) HIPCHK(c, hipMemcpyAsync(s->pred_cov.p, covs + (size_t)p0 * m * m, sizeof(double) * (size_t)m * m * Pc, hipMemcpyHostToDevice, st));
    else HIPCHK(c, hipMemcpyAsync(s->pred_var.p, vars + (size_t)p0 * m, sizeof(double) * (size_t)m * Pc, hipMemcpyHostToDevice, st));
    if (const int rc = mix_chunk(c, s, st, mp, p0, Pc, s->pred_mean.as<double>(), covs ? nullptr : s->pred_var.as<double>(),
                                 covs ? s->pred_cov.as<double>() : nullptr))
      return rc;
  }
  return mix_finish(c, s, st, mp);
}

}  // namespace

extern "C" {

int agp_mixture_moments(agp_ctx* c, int64_t m, int32_t P, const double* means, const double* vars, const double* covs,
                        const double* weights, int32_t space, double* out_mean, double* out_var, double* out_cov) {
  return abi_guard(c, [&]() -> int {
    if (const int rc = check_mixture(c, m, P, weights, space, out_cov != nullptr)) return rc;
    if (!covs && out_cov) return fail(c, AGP_ERR_ARG, "out_cov needs the components' covariances");
    if (m == 0) return AGP_OK;
    if (!means || (!vars && !covs) || !out_mean || !out_var) return fail(c, AGP_ERR_ARG, "null pointer argument");
    MixPass mp;
    mp.space = space; mp.cov = out_cov != nullptr;
    mp.out_mean = out_mean; mp.out_var = out_var; mp.out_cov = out_cov;
    // (covariances given but only mean and var wanted: their diagonals are the variances — nothing but the diagonals travels)
    std::vector<double> diag;
    if (covs && !out_cov) {
      diag.resize((size_t)m * P);
      for (int32_t p = 0; p < P; ++p)
        for (int64_t i = 0; i < m; ++i) diag[(size_t)p * m + i] = covs[(size_t)p * m * m + (size_t)i * (m + 1)];
      vars = diag.data(); covs = nullptr;
    }
    return mixture_core(c, m, P, means, vars, covs, weights, mp);
  });
}


int agp_get_mixture_stats(agp_ctx* c, int64_t* n_passes, int64_t* n_chunks) {
  if (!c || !n_passes || !n_chunks) return fail(c, AGP_ERR_ARG, "null pointer");
  std::lock_guard<std::mutex> g(c->mu);
  *n_passes = c->n_mix_passes; *n_chunks = c->n_mix_chunks;
  return AGP_OK;
}

int agp_predict_mixture_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, int32_t P, const int32_t* op_off,
                              const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                              const double* noise_pred, const double* mean_train, const double* mean_pred, const double* weights,
                              double y_slope, double y_intercept, int32_t space, double* out_mean, double* out_var, double* out_cov,
                              int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    if (const int rc = check_mixture(c, m, P, weights, space, out_cov != nullptr)) return rc;
    if (n < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if (const int rc = check_resident(c, n)) return rc;
    if (const int rc = check_y_transform(c, y_slope, y_intercept)) return rc;
    if (m == 0) return AGP_OK;
    const PredQuery q{n, ts_pred, m, mean_train, mean_pred};
    const Particles pp{P, op_off, ops, prm_off, prm, noise, noise_pred};
    if (!pp.complete() || !ts_pred || !out_mean || !out_var) return fail(c, AGP_ERR_ARG, "null pointer argument");
    MixPass mp;
    mp.space = space; mp.slope = y_slope; mp.intercept = y_intercept; mp.cov = out_cov != nullptr;
    mp.out_mean = out_mean; mp.out_var = out_var; mp.out_cov = out_cov;
    std::vector<int32_t> info((size_t)P, 0);
    int rc;
    if (out_cov) {
      rc = predict_mixture_cov(c, q, pp, weights, mp, info.data());
      if (rc) return rc;
    } else {
      // the marginal pass (out_cov = NULL: structured, lattice, store-reuse, duplicate-query and dedup paths as agp_predict_batch),
      // staged on the host as agp_predict_quantile_batch stages it
      const size_t nc = (size_t)m * P;
      std::vector<double> mean(nc), var(nc);
      rc = predict_batch(c, q, pp, mean.data(), var.data(), nullptr, info.data());
      if (rc) return rc;
      if (std::none_of(info.begin(), info.end(), [](int32_t v) { return v != 0; })) {
        rc = mixture_core(c, m, P, mean.data(), var.data(), nullptr, weights, mp);
        if (rc) return rc;
      }
    }
    if (out_info) std::copy(info.begin(), info.end(), out_info);
    // a particle without a predictive: the mixture is undefined (the reference throws building that particle's MvNormal)
    if (std::any_of(info.begin(), info.end(), [](int32_t v) { return v != 0; })) fill_nan(mp, m);
    return AGP_OK;
  });
}

}  // extern "C"
