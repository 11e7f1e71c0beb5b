// Host side of the mixture quantiles: Statistics.quantile(::MixtureModel, q; tol, max_iter) (src/api.jl:559-596) on components the
// caller supplies (agp_mixture_quantile), and predict_quantile (src/api.jl:547-557) on the resident series
// (agp_predict_quantile_batch: the marginal pass of agp_predict_batch, the raw-space transform of predict_mvn, then the search).
// The search itself is k_mixture_quantile (csrc/agp_quantile_kernel.hpp).
#include "agp_host.hpp"

#include <cfloat>

// MixtureModel's isprobvec (from memory): finite, non-negative weights whose sum isapprox 1 (rtol sqrt(eps))
int check_weights(agp_ctx* c, int32_t P, const double* w) {
  if (!w) return fail(c, AGP_ERR_ARG, "null weights");
  double s = 0.0;
  for (int32_t p = 0; p < P; ++p) {
    if (!(std::isfinite(w[p]) && w[p] >= 0.0)) return fail(c, AGP_ERR_ARG, "weights must be finite and >= 0");
    s += w[p];
  }
  if (!(std::fabs(s - 1.0) <= std::sqrt(DBL_EPSILON) * std::max(std::fabs(s), 1.0)))
    return fail(c, AGP_ERR_ARG, "weights must sum to 1");
  return AGP_OK;
}

namespace {

// the checks both entries share (predict_quantile's own: 0 < q < 1)
int check_common(agp_ctx* c, int64_t m, int32_t P, const double* weights, const double* q, int64_t nq) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (P <= 0) return fail(c, AGP_ERR_ARG, "P must be >= 1");
  if (m < 0 || nq < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (!q && nq > 0) return fail(c, AGP_ERR_ARG, "null q");
  for (int64_t k = 0; k < nq; ++k)
    if (!(q[k] > 0.0 && q[k] < 1.0)) return fail(c, AGP_ERR_ARG, "quantile must be in (0, 1)");
  const int64_t Pp = ((int64_t)P + 63) / 64 * 64;
  if (m * Pp >= ((int64_t)1 << 31) || m * nq >= ((int64_t)1 << 31)) return fail(c, AGP_ERR_ARG, "m * P or m * nq too large");
  return check_weights(c, P, weights);
}

// the device part: components (column-major m x P, as agp_predict_batch writes its means) -> x, converged, iterations
int mixture_core(agp_ctx* c, int64_t m, int32_t P, const double* means, const double* vars, const double* weights, const double* q,
                 int64_t nq, double tol, int64_t max_iter, double* out_x, int32_t* out_conv, int32_t* out_iters) {
  HIPCHK(c, hipSetDevice(c->device));
  const int Pp = (P + 63) / 64 * 64;
  const size_t nc = (size_t)m * P, np_ = (size_t)m * Pp, no = (size_t)m * nq;
  // values: the components, their packed rows, the weights, q and x; never: the converged flags and iteration counts
  struct Bufs {
    DevBuf mean{Fill::values}, var{Fill::values}, cm{Fill::values}, cs{Fill::values}, w{Fill::values}, q{Fill::values}, x{Fill::values};
    DevBuf conv{Fill::never}, iters{Fill::never};
    ~Bufs() { for (DevBuf* b : {&mean, &var, &cm, &cs, &w, &q, &x, &conv, &iters}) b->release(); }
  } b;
  for (DevBuf* d : {&b.mean, &b.var, &b.cm, &b.cs, &b.w, &b.q, &b.x}) d->pz = &c->poison;
  HIPCHK(c, b.mean.ensure(sizeof(double) * nc));
  HIPCHK(c, b.var.ensure(sizeof(double) * nc));
  HIPCHK(c, b.cm.ensure(sizeof(double) * np_));
  HIPCHK(c, b.cs.ensure(sizeof(double) * np_));
  HIPCHK(c, b.w.ensure(sizeof(double) * Pp));
  HIPCHK(c, b.q.ensure(sizeof(double) * nq));
  HIPCHK(c, b.x.ensure(sizeof(double) * no));
  if (out_conv) HIPCHK(c, b.conv.ensure(sizeof(int32_t) * no));
  if (out_iters) HIPCHK(c, b.iters.ensure(sizeof(int32_t) * no));
  std::vector<double> wp((size_t)Pp, 0.0);
  std::copy(weights, weights + P, wp.begin());
  HIPCHK(c, hipMemcpy(b.mean.p, means, sizeof(double) * nc, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.var.p, vars, sizeof(double) * nc, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.w.p, wp.data(), sizeof(double) * Pp, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(b.q.p, q, sizeof(double) * nq, hipMemcpyHostToDevice));
  launch_mixture_pack(nullptr, b.mean.as<double>(), b.var.as<double>(), P, Pp, (int)m, b.cm.as<double>(), b.cs.as<double>());
  HIPCHK(c, hipGetLastError());
  launch_mixture_quantile(nullptr, b.cm.as<double>(), b.cs.as<double>(), b.w.as<double>(), Pp, (int)m, b.q.as<double>(), (int)nq, tol,
                          (long long)max_iter, b.x.as<double>(), out_conv ? b.conv.as<int32_t>() : nullptr,
                          out_iters ? b.iters.as<int32_t>() : nullptr);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpy(out_x, b.x.p, sizeof(double) * no, hipMemcpyDeviceToHost));
  if (out_conv) HIPCHK(c, hipMemcpy(out_conv, b.conv.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
  if (out_iters) HIPCHK(c, hipMemcpy(out_iters, b.iters.p, sizeof(int32_t) * no, hipMemcpyDeviceToHost));
  return AGP_OK;
}

}  // namespace

extern "C" {

int agp_mixture_quantile(agp_ctx* c, int64_t m, int32_t P, const double* means, const double* vars, const double* weights,
                         const double* q, int64_t nq, double tol, int64_t max_iter, double* out_x, int32_t* out_converged,
                         int32_t* out_iters) {
  return abi_guard(c, [&]() -> int {
    int rc = check_common(c, m, P, weights, q, nq);
    if (rc) return rc;
    if (m == 0 || nq == 0) return AGP_OK;
    if (!means || !vars || !out_x) return fail(c, AGP_ERR_ARG, "null pointer argument");
    // Normal(mu, sqrt(v)) of the reference throws on these; components at weight 0 are never evaluated
    for (int32_t p = 0; p < P; ++p) {
      if (weights[p] == 0.0) continue;
      for (int64_t i = 0; i < m; ++i) {
        const double mu = means[(size_t)p * m + i], v = vars[(size_t)p * m + i];
        if (!std::isfinite(mu)) return fail(c, AGP_ERR_ARG, "non-finite component mean at positive weight");
        if (!(v >= 0.0)) return fail(c, AGP_ERR_ARG, "negative or NaN component variance at positive weight");
      }
    }
    return mixture_core(c, m, P, means, vars, weights, q, nq, tol, max_iter, out_x, out_converged, out_iters);
  });
}


int agp_predict_quantile_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, int32_t P, const int32_t* op_off,
                               const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                               const double* noise_pred, const double* mean_train, const double* mean_pred, const double* weights,
                               double y_slope, double y_intercept, const double* q, int64_t nq, double tol, int64_t max_iter,
                               double* out_x, int32_t* out_converged, int32_t* out_iters, int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    int rc = check_common(c, m, P, weights, q, nq);
    if (rc) return rc;
    if (n < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if ((rc = check_y_transform(c, y_slope, y_intercept))) return rc;
    if (m == 0 || nq == 0) return AGP_OK;
    if (!out_x) return fail(c, AGP_ERR_ARG, "null pointer argument");
    // the marginal pass (out_cov = NULL: structured, lattice, store-reuse and dedup paths as agp_predict_batch), staged on the host
    const size_t nc = (size_t)m * P;
    std::vector<double> mean(nc), var(nc);
    std::vector<int32_t> info((size_t)P, 0);
    rc = predict_batch(c, {n, ts_pred, m, mean_train, mean_pred}, {P, op_off, ops, prm_off, prm, noise, noise_pred}, mean.data(), var.data(),
                       nullptr, info.data());
    if (rc) return rc;
    // raw space (predict_mvn, src/api.jl:513-520; Transforms.jl:44-49): (mu - intercept) / slope, (1 / slope^2) * var
    const double iv = 1.0 / (y_slope * y_slope);
    bool bad = false;
    for (int32_t p = 0; p < P; ++p) {
      double* mp = mean.data() + (size_t)p * m;
      double* vp = var.data() + (size_t)p * m;
      for (int64_t i = 0; i < m; ++i) {
        mp[i] = (mp[i] - y_intercept) / y_slope;
        vp[i] = iv * vp[i];
        if (info[(size_t)p] == 0 && !(std::isfinite(mp[i]) && vp[i] >= 0.0)) info[(size_t)p] = (int32_t)(n + i + 1);
      }
      bad = bad || info[(size_t)p] != 0;
    }
    if (out_info) std::copy(info.begin(), info.end(), out_info);
    if (bad) {
      // a particle without a predictive: the mixture is undefined (the reference throws) — NaN everywhere, nothing converged
      const size_t no = (size_t)m * nq;
      std::fill(out_x, out_x + no, std::numeric_limits<double>::quiet_NaN());
      if (out_converged) std::fill(out_converged, out_converged + no, 0);
      if (out_iters) std::fill(out_iters, out_iters + no, 0);
      return AGP_OK;
    }
    return mixture_core(c, m, P, mean.data(), var.data(), weights, q, nq, tol, max_iter, out_x, out_converged, out_iters);
  });
}

}  // extern "C"
