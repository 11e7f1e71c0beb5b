// agp_logpdf_series_batch: many SHORT series, each with its own particles, scored in one call by the small-matrix value kernel
// (agp_series_kernel.hpp: one workgroup per particle, covariance + Cholesky + forward solve + value in LDS), and
// agp_logpdf_grad_series_batch, its value-and-gradient twin (k_series_logpdf_grad: L^-T, alpha and the contraction with dK / d theta
// behind the value, same workgroup, same LDS), and agp_predict_series_batch, its predictive twin (k_series_predict: posterior mean and
// marginal variance at every series' own query times from the factor the value has just left in LDS), and
// agp_predict_quantile_series_batch, the forecast band on top of it (the predictive launches' device outputs read out by
// agp_series_quantile_kernel.hpp on the same stream: quantiles and marginal moments of every series' own mixture).  All four are one
// host function — validation, series upload, launch classes and the value outputs are the same statements — with the gradient, the
// prediction and the band as options.  Stateless: the series
// travel with the call; the resident series, its tables, the factor store, the coalescer and every counter of the context are
// neither read nor changed — only a workspace slot (stream, staging buffers) is borrowed, as in every batch entry.
#include "agp_host.hpp"

static_assert(SERIES_MAX_N == AGP_SERIES_MAX_N, "the kernel's cap is the C ABI's");
static_assert(AGP_SERIES_MAX_N >= 160, "the reference's 126-, 135-, 143- and 144-point series must fit");

namespace {

// LDS classes of the launches: a launch declares the largest need of its particles, so particles are grouped by how many workgroups
// of their size share a CU's 160 KiB — 4 (n <= ~80), 2 (n <= ~128) or 1.
int lds_class(size_t bytes) { return bytes <= (size_t)SERIES_LDS_BYTES / 4 ? 0 : bytes <= (size_t)SERIES_LDS_BYTES / 2 ? 1 : 2; }

// The prediction of agp_predict_series_batch: every series' query times and the particle-major outputs (host).
struct SeriesPredOut {
  const int64_t* q_off;      // [S + 1]
  const double* ts_pred;
  double* mean;              // [off[P]]
  double* var;
  int64_t* off;              // [P + 1], written by the entry
};

// The band of agp_predict_quantile_series_batch: the mixtures' weights and transforms, the quantiles, and the outputs (host).
struct SeriesQuantOut {
  const double* weights;     // [P] particle p's weight inside its series' mixture
  const double* y_slope;     // [S] or null (1)
  const double* y_intercept; // [S] or null (0)
  const double* q; int64_t nq; double tol; int64_t max_iter;
  double* x; int32_t* conv; int32_t* iters;      // [nq q_off[S]]; conv / iters nullable
  double* mix_mean; double* mix_var;              // [q_off[S]], nullable
};

// What the read-out kernels index with, built and checked on the host before anything is launched or written.
struct QuantPlan {
  std::vector<long long> tab;      // [pl_off (S + 1) | w_off (S + 1) | row_off (S + 1)]
  std::vector<int32_t> plist;      // [P] the series' particles, series by series, ascending within each
  std::vector<double> vals;        // [w (w_off[S], 0 in the padding) | slope (S) | intercept (S) | ivar (S) | q (nq)]
  long long max_rows_el = 0;       // largest m_s Pp_s
  size_t Q = 0, R = 0, W = 0;      // q_off[S], row_off[S], w_off[S]
};

// prefixes the message a shared check has just stored with the series it was about
int fail_series(agp_ctx* c, int rc, int32_t s) {
  std::string msg;
  { std::lock_guard<std::mutex> g(c->mu); msg = c->err; }
  return fail(c, rc, "series " + std::to_string(s) + ": " + msg);
}

int quant_plan(agp_ctx* c, int32_t S, int P, const int32_t* series, const int64_t* q_off, const SeriesQuantOut& qo, QuantPlan& pl) {
  if (qo.nq < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (!qo.q && qo.nq > 0) return fail(c, AGP_ERR_ARG, "null q");
  for (int64_t k = 0; k < qo.nq; ++k)
    if (!(qo.q[k] > 0.0 && qo.q[k] < 1.0)) return fail(c, AGP_ERR_ARG, "quantile must be in (0, 1)");
  if (!qo.x && qo.nq > 0) return fail(c, AGP_ERR_ARG, "null pointer argument (out_x)");
  if (!qo.weights && P > 0) return fail(c, AGP_ERR_ARG, "null weights");
  pl.Q = S > 0 ? (size_t)q_off[S] : 0;
  if ((int64_t)pl.Q >= ((int64_t)1 << 31) || (qo.nq > 0 && (int64_t)pl.Q * qo.nq >= ((int64_t)1 << 31)))
    return fail(c, AGP_ERR_ARG, "nq * q_off[S] too large");
  const size_t S1 = (size_t)S + 1;
  pl.tab.assign(3 * S1, 0);
  long long* pl_off = pl.tab.data();
  long long* w_off = pl_off + S1;
  long long* row_off = w_off + S1;
  for (int p = 0; p < P; ++p) ++pl_off[series[p] + 1];
  for (int32_t s = 0; s < S; ++s) pl_off[s + 1] += pl_off[s];
  pl.plist.resize((size_t)P);
  {
    std::vector<long long> at(pl_off, pl_off + S);
    for (int p = 0; p < P; ++p) pl.plist[(size_t)at[(size_t)series[p]]++] = p;
  }
  for (int32_t s = 0; s < S; ++s) {
    const long long Ps = pl_off[s + 1] - pl_off[s], Pp = (Ps + 63) / 64 * 64, m = q_off[s + 1] - q_off[s];
    w_off[s + 1] = w_off[s] + Pp;
    row_off[s + 1] = row_off[s] + m * Pp;      // (m <= 2^30, Pp < 2^31 + 64: no overflow before the test)
    if (row_off[s + 1] >= ((long long)1 << 31) || w_off[s + 1] >= ((long long)1 << 31))
      return fail(c, AGP_ERR_ARG, "sum over the series of m_s * ceil(P_s / 64) * 64 too large");
    pl.max_rows_el = std::max(pl.max_rows_el, m * Pp);
  }
  pl.W = (size_t)w_off[S]; pl.R = (size_t)row_off[S];
  pl.vals.assign(pl.W + 3 * (size_t)S + (size_t)qo.nq, 0.0);
  double* w = pl.vals.data();
  double* slope = w + pl.W;
  double* icpt = slope + S;
  double* ivar = icpt + S;
  std::vector<double> ws;
  for (int32_t s = 0; s < S; ++s) {
    slope[s] = qo.y_slope ? qo.y_slope[s] : 1.0;
    icpt[s] = qo.y_intercept ? qo.y_intercept[s] : 0.0;
    if (const int rc = check_y_transform(c, slope[s], icpt[s])) return fail_series(c, rc, s);
    ivar[s] = 1.0 / (slope[s] * slope[s]);
    const long long Ps = pl_off[s + 1] - pl_off[s];
    if (Ps == 0) continue;
    ws.resize((size_t)Ps);
    for (long long j = 0; j < Ps; ++j) ws[(size_t)j] = qo.weights[pl.plist[(size_t)(pl_off[s] + j)]];
    if (const int rc = check_weights(c, (int32_t)Ps, ws.data())) return fail_series(c, rc, s);
    std::copy(ws.begin(), ws.end(), w + w_off[s]);
  }
  std::copy(qo.q, qo.q + qo.nq, ivar + S);
  return AGP_OK;
}

// a band without a mixture behind it: NaN, nothing converged
void quant_fill_nan(const SeriesQuantOut& qo, size_t from, size_t to, int64_t nq) {
  const double nanv = std::numeric_limits<double>::quiet_NaN();
  if (qo.x) std::fill(qo.x + from * nq, qo.x + to * nq, nanv);
  if (qo.conv) std::fill(qo.conv + from * nq, qo.conv + to * nq, 0);
  if (qo.iters) std::fill(qo.iters + from * nq, qo.iters + to * nq, 0);
  if (qo.mix_mean) std::fill(qo.mix_mean + from, qo.mix_mean + to, nanv);
  if (qo.mix_var) std::fill(qo.mix_var + from, qo.mix_var + to, nanv);
}

// go = null, po = null: values only.  go: also out_grad (agp_logpdf_grad_batch's layout) and out_gnoise.  po: also the posterior at
// the series' query times; out_logpdf may then be null (pp.noise_pred null: the particle's own noise).  qo (with po, whose mean / var / off
// are then null: the per-particle predictive stays on the device): the band of every series' mixture instead.
int series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, const Particles& pp,
                 const int32_t* series, double* out_logpdf, int32_t* out_info, const GradOut* go = nullptr,
                 const SeriesPredOut* po = nullptr, const SeriesQuantOut* qo = nullptr) {
  const int P = pp.P;
  char buf[256];
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (S < 0 || P < 0) return fail(c, AGP_ERR_ARG, "negative number of series or particles");
  if (P == 0 && !qo) return AGP_OK;
  if (!pt_off || !ts || !xs || !series || !pp.complete() || (!out_logpdf && !po) || !out_info) return fail(c, AGP_ERR_ARG, "null pointer argument");
  if (po && (!po->q_off || !po->ts_pred || (!qo && (!po->mean || !po->var || !po->off))))
    return fail(c, AGP_ERR_ARG, "null pointer argument (q_off, ts_pred, out_mean, out_var or out_off)");
  const size_t n_prm_total = go ? (size_t)std::max(0, pp.prm_off[P]) : 0;
  if (go && !go->gnoise) return fail(c, AGP_ERR_ARG, "null pointer argument (out_grad_noise)");
  if (go && !go->grad && pp.prm_off[P] > 0) return fail(c, AGP_ERR_ARG, "null pointer argument (out_grad with parameters present)");
  if (S > 0 && pt_off[0] != 0) return fail(c, AGP_ERR_ARG, "pt_off[0] must be 0 (series 0)");
  for (int32_t s = 0; s < S; ++s) {
    if (pt_off[s + 1] < pt_off[s]) {
      snprintf(buf, sizeof buf, "series %d: pt_off decreases (%lld after %lld)", (int)s, (long long)pt_off[s + 1], (long long)pt_off[s]);
      return fail(c, AGP_ERR_ARG, buf);
    }
    if (pt_off[s + 1] - pt_off[s] > AGP_SERIES_MAX_N) {
      snprintf(buf, sizeof buf, "series %d has %lld points, more than AGP_SERIES_MAX_N (%d)", (int)s, (long long)(pt_off[s + 1] - pt_off[s]),
               AGP_SERIES_MAX_N);
      return fail(c, AGP_ERR_ARG, buf);
    }
  }
  if (po) {
    if (S > 0 && po->q_off[0] != 0) return fail(c, AGP_ERR_ARG, "q_off[0] must be 0 (series 0)");
    for (int32_t s = 0; s < S; ++s) {
      if (po->q_off[s + 1] < po->q_off[s]) {
        snprintf(buf, sizeof buf, "series %d: q_off decreases (%lld after %lld)", (int)s, (long long)po->q_off[s + 1], (long long)po->q_off[s]);
        return fail(c, AGP_ERR_ARG, buf);
      }
      if (po->q_off[s + 1] - po->q_off[s] > (int64_t)1 << 30) {
        snprintf(buf, sizeof buf, "series %d has %lld query points, more than 2^30", (int)s, (long long)(po->q_off[s + 1] - po->q_off[s]));
        return fail(c, AGP_ERR_ARG, buf);
      }
    }
  }
  for (int p = 0; p < P; ++p)
    if (series[p] < 0 || series[p] >= S) {
      snprintf(buf, sizeof buf, "particle %d: series index %d outside [0, %d)", p, (int)series[p], (int)S);
      return fail(c, AGP_ERR_ARG, buf);
    }
  for (int p = 0; p < P; ++p)
    if (pp.op_off[p] < 0 || pp.prm_off[p] < 0 || pp.op_off[p + 1] < pp.op_off[p] || pp.prm_off[p + 1] < pp.prm_off[p]) {
      snprintf(buf, sizeof buf, "particle %d: malformed program / parameter offsets", p);
      return fail(c, AGP_ERR_ARG, buf);
    }
  QuantPlan qp;
  if (qo) {
    if (const int rc = quant_plan(c, S, P, series, po->q_off, *qo, qp)) return rc;
    if (P == 0) { quant_fill_nan(*qo, 0, qp.Q, qo->nq); return AGP_OK; }      // (S series without a particle)
  }
  // programs without any table of the resident series (no log|dt| table, no lag tables), in the caller's order
  Batch bt;
  CompileOpts co;
  co.ge_tab = false; co.lag = false; co.never_fuse = true; co.want_grad = go != nullptr;
  if (const int rc = compile_batch(c, pp, bt, co)) return rc;
  if (go)
    for (int p = 0; p < P; ++p)
      if (bt.ghdr[(size_t)p].n_ops > 64) {      // (RegTape<64> is the largest tape: agp_logpdf_grad_batch's own limit)
        snprintf(buf, sizeof buf, "particle %d: gradient supports kernel trees of up to 64 nodes (%d)", p, (int)bt.ghdr[(size_t)p].n_ops);
        return fail(c, AGP_ERR_PROGRAM, buf);
      }

  // per particle: length, LDS need; launch classes (kernel instantiation) x (LDS class), longest series first inside each.
  // Instantiations: values — evaluation-stack depth 4 / 8; gradient — tape of 16 / 64 nodes, the 64-node tape with the depth the value
  // entry picks for the same program (<= 16 nodes never need more than 4), so that the value's bits are that entry's
  std::vector<int> len((size_t)P);
  std::vector<size_t> need((size_t)P);
  std::vector<int64_t> nq((size_t)P, 0);      // query points of the particle's series (prediction)
  std::vector<int32_t> list[3][3];
  for (int p = 0; p < P; ++p) {
    if (bt.order[(size_t)p] != p) return fail(c, AGP_ERR_HOST, "internal error: compiled batch out of order");
    const ProgHdr& h = bt.hdr[(size_t)p];
    const int n = (int)(pt_off[series[p] + 1] - pt_off[series[p]]);
    len[(size_t)p] = n;
    if (po) nq[(size_t)p] = po->q_off[series[p] + 1] - po->q_off[series[p]];
    if (n == 0 && nq[(size_t)p] == 0) continue;      // (an empty series is launched for its prior predictive only)
    const int m_total = go ? series_grad_lds(n, h.n_ops, h.n_prm, h.n_cp, bt.ghdr[(size_t)p].n_ops, bt.ghdr[(size_t)p].n_prm).total
                        : po ? series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp).total
                             : series_lds(n, h.n_ops, h.n_prm, h.n_cp).total;
    need[(size_t)p] = sizeof(double) * (size_t)m_total;
    if (need[(size_t)p] > (size_t)SERIES_LDS_BYTES) {
      snprintf(buf, sizeof buf, "particle %d: %d per-point tables (ChangePoint nodes) at %d points need %zu bytes of LDS, more than the "
               "kernel's %d", p, (int)h.n_cp, n, need[(size_t)p], SERIES_LDS_BYTES);
      return fail(c, AGP_ERR_PROGRAM, buf);
    }
    // the evaluation stack this program needs (compile_batch reports the batch's largest only): from the compiled postfix form
    int sp = 0, depth = 0;
    for (int i = 0; i < h.n_ops; ++i) {
      const int o = bt.ops[(size_t)h.op_off + i];
      if (o == OP_PLUS || o == OP_TIMES || o == OP_CP || o == OP_CP_SWAP) --sp; else ++sp;
      depth = std::max(depth, sp);
    }
    const int inst = !go ? (depth <= 4 ? 0 : 1) : bt.ghdr[(size_t)p].n_ops <= 16 && depth <= 4 ? 0 : depth <= 4 ? 1 : 2;
    list[inst][lds_class(need[(size_t)p])].push_back(p);
  }
  for (auto& ld : list)
    for (auto& v : ld) std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) { return len[(size_t)x] > len[(size_t)y]; });
  std::vector<int32_t> wg;
  wg.reserve((size_t)P);
  for (auto& ld : list) for (auto& v : ld) wg.insert(wg.end(), v.begin(), v.end());
  std::vector<long long> ooff;      // out_off: the particle-major layout of the prediction
  if (po) {
    ooff.assign((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) ooff[(size_t)p + 1] = ooff[(size_t)p] + nq[(size_t)p];
    if (po->off) std::copy(ooff.begin(), ooff.end(), po->off);
  }
  const size_t n_out = po ? (size_t)ooff[(size_t)P] : 0;
  if (wg.empty()) {      // every particle scores an empty series (src/inference_smc_anneal_data.jl:185-187) and has nothing to predict
    if (out_logpdf) std::fill(out_logpdf, out_logpdf + P, 0.0);
    std::fill(out_info, out_info + P, 0);
    if (go) { std::fill(go->gnoise, go->gnoise + P, 0.0); std::fill(go->grad, go->grad + n_prm_total, 0.0); }
    if (qo) quant_fill_nan(*qo, 0, qp.Q, qo->nq);      // (only series without a particle have query points here)
    return AGP_OK;
  }

  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const size_t npts = (size_t)pt_off[S];
  // device buffers of the slot: programs as in every sweep; tt = [ts | xs]; map = [pt_off (int64) | series | wg]
  const size_t o_series = sizeof(long long) * ((size_t)S + 1), o_wg = o_series + sizeof(int32_t) * (size_t)P;
  HIPCHK(c, s->hdr.ensure(sizeof(ProgHdr) * (size_t)P));
  HIPCHK(c, s->ops.ensure(bt.ops.size() + 4));
  HIPCHK(c, s->prm.ensure(sizeof(double) * std::max<size_t>(1, bt.prm.size())));
  HIPCHK(c, s->noise.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->tt.ensure(sizeof(double) * 2 * std::max<size_t>(1, npts)));
  HIPCHK(c, s->map.ensure(o_wg + sizeof(int32_t) * wg.size()));
  HIPCHK(c, s->out_lp.ensure(sizeof(double) * (size_t)P + sizeof(int32_t) * (size_t)P));
  if (go) {
    HIPCHK(c, s->ghdr.ensure(sizeof(GProgHdr) * (size_t)P));
    HIPCHK(c, s->gops.ensure(bt.gops.size() + 4));
    HIPCHK(c, s->glc.ensure(bt.glc.size() + 4));
    HIPCHK(c, s->grc.ensure(bt.grc.size() + 4));
    HIPCHK(c, s->gpoff.ensure(sizeof(int32_t) * (bt.gpoff.size() + 1)));
    HIPCHK(c, s->gprm.ensure(sizeof(double) * bt.gprm.size()));
    HIPCHK(c, s->gmap.ensure(sizeof(int32_t) * (bt.gmap.size() + 1)));
    HIPCHK(c, s->goff.ensure(sizeof(int32_t) * (size_t)P));
    HIPCHK(c, s->dgrad.ensure(sizeof(double) * std::max<size_t>(1, n_prm_total)));
    HIPCHK(c, s->dgnoise.ensure(sizeof(double) * (size_t)P));
  }
  const size_t nqt = po ? (size_t)po->q_off[S] : 0;
  const size_t o_qoff = (o_wg + sizeof(int32_t) * wg.size() + 7) & ~(size_t)7, o_ooff = o_qoff + sizeof(long long) * ((size_t)S + 1);
  if (po) {      // tt = [ts | xs | ts_pred]; map = [.. | q_off (int64) | out_off (int64)]; outputs in pred_mean / pred_var
    HIPCHK(c, s->tt.ensure(sizeof(double) * (2 * std::max<size_t>(1, npts) + std::max<size_t>(1, nqt))));
    HIPCHK(c, s->map.ensure(o_ooff + sizeof(long long) * ((size_t)P + 1)));
    HIPCHK(c, s->noise_pred.ensure(sizeof(double) * (size_t)P));
    HIPCHK(c, s->pred_mean.ensure(sizeof(double) * std::max<size_t>(1, n_out)));
    HIPCHK(c, s->pred_var.ensure(sizeof(double) * std::max<size_t>(1, n_out)));
  }
  // the band: x and the moments in sq_out, the flags in sq_flag = [converged | iterations | first_bad (P) | bad (S)]
  const size_t nx = qo ? qp.Q * (size_t)qo->nq : 0;
  const bool want_mom = qo && (qo->mix_mean || qo->mix_var);
  const size_t S1 = (size_t)S + 1, o_plist = sizeof(long long) * 3 * S1;
  if (qo) {
    HIPCHK(c, s->sq_tab.ensure(o_plist + sizeof(int32_t) * (size_t)P));
    HIPCHK(c, s->sq_w.ensure(sizeof(double) * std::max<size_t>(1, qp.vals.size())));
    HIPCHK(c, s->sq_cm.ensure(sizeof(double) * std::max<size_t>(1, qp.R)));
    HIPCHK(c, s->sq_cs.ensure(sizeof(double) * std::max<size_t>(1, qp.R)));
    HIPCHK(c, s->sq_out.ensure(sizeof(double) * std::max<size_t>(1, nx + 2 * qp.Q)));
    HIPCHK(c, s->sq_flag.ensure(sizeof(int32_t) * (2 * nx + (size_t)P + (size_t)S)));
  }
  std::vector<long long> off64(pt_off, pt_off + S + 1);
  PinnedUploads up;
  up.add(s->hdr.p, bt.hdr.data(), sizeof(ProgHdr) * (size_t)P);
  up.add(s->ops.p, bt.ops.data(), bt.ops.size());
  up.add(s->prm.p, bt.prm.data(), sizeof(double) * bt.prm.size());
  up.add(s->noise.p, pp.noise, sizeof(double) * (size_t)P);
  up.add(s->tt.p, ts, sizeof(double) * npts);
  up.add(s->tt.as<double>() + npts, xs, sizeof(double) * npts);
  up.add(s->map.p, off64.data(), o_series);
  up.add(s->map.as<char>() + o_series, series, sizeof(int32_t) * (size_t)P);
  up.add(s->map.as<char>() + o_wg, wg.data(), sizeof(int32_t) * wg.size());
  if (go) {
    up.add(s->ghdr.p, bt.ghdr.data(), sizeof(GProgHdr) * (size_t)P);
    up.add(s->gops.p, bt.gops.data(), bt.gops.size());
    up.add(s->glc.p, bt.glc.data(), bt.glc.size());
    up.add(s->grc.p, bt.grc.data(), bt.grc.size());
    up.add(s->gpoff.p, bt.gpoff.data(), sizeof(int32_t) * bt.gpoff.size());
    up.add(s->gprm.p, bt.gprm.data(), sizeof(double) * bt.gprm.size());
    up.add(s->gmap.p, bt.gmap.data(), sizeof(int32_t) * bt.gmap.size());
    up.add(s->goff.p, pp.prm_off, sizeof(int32_t) * (size_t)P);      // the particle's block in out_grad: the caller's own offsets
  }
  std::vector<long long> qoff64;
  if (po) {
    qoff64.assign(po->q_off, po->q_off + S + 1);
    up.add(s->map.as<char>() + o_qoff, qoff64.data(), sizeof(long long) * ((size_t)S + 1));
    up.add(s->map.as<char>() + o_ooff, ooff.data(), sizeof(long long) * ((size_t)P + 1));
    up.add(s->tt.as<double>() + 2 * npts, po->ts_pred, sizeof(double) * nqt);
    up.add(s->noise_pred.p, pp.noise_pred ? pp.noise_pred : pp.noise, sizeof(double) * (size_t)P);
  }
  if (qo) {
    up.add(s->sq_tab.p, qp.tab.data(), o_plist);
    up.add(s->sq_tab.as<char>() + o_plist, qp.plist.data(), sizeof(int32_t) * (size_t)P);
    up.add(s->sq_w.p, qp.vals.data(), sizeof(double) * qp.vals.size());
  }
  HIPCHK(c, up.flush(s->h_stage, s->up_blob, st));

  SeriesGradArgs sa = {};      // (the value launches take its SeriesArgs part)
  if (go) {
    sa.ghdr = s->ghdr.as<GProgHdr>(); sa.gops = s->gops.as<uint8_t>(); sa.glc = s->glc.as<uint8_t>(); sa.grc = s->grc.as<uint8_t>();
    sa.gpoff = s->gpoff.as<int32_t>(); sa.gprm = s->gprm.as<double>(); sa.gmap = s->gmap.as<int32_t>();
    sa.out_off = s->goff.as<int32_t>(); sa.out_grad = s->dgrad.as<double>(); sa.out_gnoise = s->dgnoise.as<double>();
  }
  sa.ts = s->tt.as<double>(); sa.xs = s->tt.as<double>() + npts;
  sa.pt_off = s->map.as<long long>();
  sa.series = reinterpret_cast<const int32_t*>(s->map.as<char>() + o_series);
  sa.hdr = s->hdr.as<ProgHdr>(); sa.ops = s->ops.as<uint8_t>(); sa.prm = s->prm.as<double>(); sa.noise = s->noise.as<double>();
  sa.out_lp = s->out_lp.as<double>(); sa.out_info = reinterpret_cast<int32_t*>(s->out_lp.as<double>() + P);
  const bool prof = c->profiling;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (prof) {
    while (s->events.size() < 3) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); s->events.push_back(e); }
    ev[0] = s->events[0]; ev[1] = s->events[1]; ev[2] = s->events[2];
    HIPCHK(c, hipEventRecord(ev[0], st));
  }
  size_t w0 = 0;
  for (int d = 0; d < 3; ++d)
    for (int k = 0; k < 3; ++k) {
      const std::vector<int32_t>& v = list[d][k];
      if (v.empty()) continue;
      size_t lds = 0;
      for (int32_t p : v) lds = std::max(lds, need[(size_t)p]);
      sa.wg = reinterpret_cast<const int32_t*>(s->map.as<char>() + o_wg) + w0;
      if (go) HIPCHK(c, launch_series_logpdf_grad(st, sa, (int)v.size(), d == 2 ? 8 : 4, d == 0 ? 16 : 64, lds));
      else if (po) {
        SeriesPredArgs spa = {};
        static_cast<SeriesArgs&>(spa) = sa;
        spa.q_off = reinterpret_cast<const long long*>(s->map.as<char>() + o_qoff);
        spa.out_off = reinterpret_cast<const long long*>(s->map.as<char>() + o_ooff);
        spa.ts_pred = s->tt.as<double>() + 2 * npts; spa.noise_pred = s->noise_pred.as<double>();
        spa.out_mean = s->pred_mean.as<double>(); spa.out_var = s->pred_var.as<double>();
        HIPCHK(c, launch_series_predict(st, spa, (int)v.size(), d == 0 ? 4 : 8, lds));
      } else HIPCHK(c, launch_series_logpdf(st, sa, (int)v.size(), d == 0 ? 4 : 8, lds));
      w0 += v.size();
    }
  if (prof) HIPCHK(c, hipEventRecord(ev[1], st));
  if (qo) {
    // the read-out, behind the predictive launches on the same stream: their means and variances never leave the device
    SeriesQuantArgs qa = {};
    qa.S = S; qa.nq = (int)qo->nq;
    qa.pt_off = sa.pt_off;
    qa.q_off = reinterpret_cast<const long long*>(s->map.as<char>() + o_qoff);
    qa.out_off = reinterpret_cast<const long long*>(s->map.as<char>() + o_ooff);
    qa.mean = s->pred_mean.as<double>(); qa.var = s->pred_var.as<double>(); qa.pred_info = sa.out_info;
    qa.pl_off = s->sq_tab.as<long long>(); qa.w_off = qa.pl_off + S1; qa.row_off = qa.w_off + S1;
    qa.plist = reinterpret_cast<const int32_t*>(s->sq_tab.as<char>() + o_plist);
    qa.w = s->sq_w.as<double>(); qa.slope = qa.w + qp.W; qa.intercept = qa.slope + S; qa.ivar = qa.intercept + S; qa.q = qa.ivar + S;
    qa.tol = qo->tol; qa.max_iter = (long long)qo->max_iter;
    qa.cm = s->sq_cm.as<double>(); qa.cs = s->sq_cs.as<double>();
    qa.out_x = s->sq_out.as<double>();
    qa.out_mean = want_mom ? qa.out_x + nx : nullptr; qa.out_var = want_mom ? qa.out_x + nx + qp.Q : nullptr;
    qa.out_conv = s->sq_flag.as<int32_t>(); qa.out_iters = qa.out_conv + nx;
    qa.first_bad = qa.out_iters + nx; qa.bad = qa.first_bad + P;
    launch_series_mix_readout(st, qa, (long long)qp.Q, qp.max_rows_el);
    HIPCHK(c, hipGetLastError());
    if (prof) HIPCHK(c, hipEventRecord(ev[2], st));
  }
  const size_t out_bytes = sizeof(double) * (size_t)P + sizeof(int32_t) * (size_t)P;
  const size_t o_gn = (out_bytes + 7) & ~(size_t)7, o_gr = o_gn + sizeof(double) * (size_t)P;      // gradient outputs behind [logpdf | info]
  const size_t n_band = nx + (want_mom ? 2 * qp.Q : 0), o_bf = o_gn + sizeof(double) * n_band;     // band: [x | mean | var], then the flags
  HIPCHK(c, s->h_out.ensure(go ? o_gr + sizeof(double) * n_prm_total : qo ? o_bf + sizeof(int32_t) * (2 * nx + (size_t)P)
                               : po ? o_gn + 2 * sizeof(double) * n_out : out_bytes));
  HIPCHK(c, hipMemcpyAsync(s->h_out.p, s->out_lp.p, out_bytes, hipMemcpyDeviceToHost, st));
  if (go) {
    char* ho = static_cast<char*>(s->h_out.p);
    HIPCHK(c, hipMemcpyAsync(ho + o_gn, s->dgnoise.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
    if (n_prm_total > 0) HIPCHK(c, hipMemcpyAsync(ho + o_gr, s->dgrad.p, sizeof(double) * n_prm_total, hipMemcpyDeviceToHost, st));
  }
  if (qo) {      // [x | mean | var | converged | iterations | first_bad] behind [logpdf | info]
    char* ho = static_cast<char*>(s->h_out.p);
    if (n_band > 0) HIPCHK(c, hipMemcpyAsync(ho + o_gn, s->sq_out.p, sizeof(double) * n_band, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ho + o_bf, s->sq_flag.p, sizeof(int32_t) * (2 * nx + (size_t)P), hipMemcpyDeviceToHost, st));
  } else if (po && n_out > 0) {      // [mean | var] behind [logpdf | info]
    char* ho = static_cast<char*>(s->h_out.p);
    HIPCHK(c, hipMemcpyAsync(ho + o_gn, s->pred_mean.p, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ho + o_gn + sizeof(double) * n_out, s->pred_var.p, sizeof(double) * n_out, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  const double* hl = static_cast<const double*>(s->h_out.p);
  const int32_t* hi = reinterpret_cast<const int32_t*>(hl + P);
  for (int p = 0; p < P; ++p) {
    const bool empty = len[(size_t)p] == 0;      // (never launched, or launched for the prior predictive: the value is 0 either way)
    if (out_logpdf) out_logpdf[p] = empty ? 0.0 : hl[p];
    out_info[p] = empty ? 0 : hi[p];
    if (go) {
      // (an empty series: zeros; a bad pivot: NaN in the whole block — the kernel wrote them, slot by slot through gmap)
      const double* hgn = reinterpret_cast<const double*>(static_cast<const char*>(s->h_out.p) + o_gn);
      const double* hgr = hgn + P;
      go->gnoise[p] = empty ? 0.0 : hgn[p];
      for (int32_t q = pp.prm_off[p]; q < pp.prm_off[p + 1]; ++q) go->grad[q] = empty ? 0.0 : hgr[q];
    }
  }
  if (qo) {
    const char* ho = static_cast<const char*>(s->h_out.p);
    const double* hb = reinterpret_cast<const double*>(ho + o_gn);
    const int32_t* hf = reinterpret_cast<const int32_t*>(ho + o_bf);
    // raw_components' rule: a particle whose predictive exists but whose raw mean or variance is unusable at query i reports n_s + i + 1
    for (int p = 0; p < P; ++p)
      if (out_info[p] == 0 && nq[(size_t)p] > 0 && hf[2 * nx + (size_t)p] != 0) out_info[p] = hf[2 * nx + (size_t)p];
    if (qo->x) std::copy(hb, hb + nx, qo->x);
    if (qo->conv) std::copy(hf, hf + nx, qo->conv);
    if (qo->iters) std::copy(hf + nx, hf + 2 * nx, qo->iters);
    if (qo->mix_mean) std::copy(hb + nx, hb + nx + qp.Q, qo->mix_mean);
    if (qo->mix_var) std::copy(hb + nx + qp.Q, hb + nx + 2 * qp.Q, qo->mix_var);
  } else if (po && n_out > 0) {      // every particle with query points was launched and wrote its whole block
    const double* hm = reinterpret_cast<const double*>(static_cast<const char*>(s->h_out.p) + o_gn);
    std::copy(hm, hm + n_out, po->mean);
    std::copy(hm + n_out, hm + 2 * n_out, po->var);
  }
  if (prof) {
    // agp_get_timing: out[0] = out[2] = the value kernels of the call (covariance, factorisation, solve and value are one kernel)
    float ms = 0.f, rd = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev[0], ev[1]));
    if (qo) HIPCHK(c, hipEventElapsedTime(&rd, ev[1], ev[2]));
    std::lock_guard<std::mutex> g(c->mu);
    for (double& t : c->timing) t = 0.0;
    c->timing[0] = ms; c->timing[2] = ms;
    c->timing[4] = rd;      // the band's three read-out kernels (0 in the other entries)
  }
  return AGP_OK;
}

// agp_debug_series_factor: P caller matrices of one size through stages 4 and 5 of the value kernel (its probe instantiation).
int series_factor(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, double* out_L, double* out_alpha,
                  double* out_part, double* out_lp, int32_t* out_info) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (n <= 0 || n > AGP_SERIES_MAX_N) {
    char buf[128];
    snprintf(buf, sizeof buf, "series probe: n = %lld outside [1, AGP_SERIES_MAX_N = %d]", (long long)n, AGP_SERIES_MAX_N);
    return fail(c, AGP_ERR_ARG, buf);
  }
  if (P <= 0 || P > (1 << 16)) return fail(c, AGP_ERR_ARG, "series probe: 1 .. 65536 matrices per call");
  if (!K || !out_L || !out_alpha || !out_part || !out_lp || !out_info) return fail(c, AGP_ERR_ARG, "null pointer argument");
  const SeriesLds m = series_lds((int)n, 0, 0, 0);
  const size_t nel = (size_t)n * n, nblk = (size_t)m.nb * (m.nb + 1) / 2, bel = nblk * 256;
  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  HIPCHK(c, s->dense.ensure(sizeof(double) * nel * P));
  if (y) HIPCHK(c, s->vec.ensure(sizeof(double) * (size_t)n * P));
  HIPCHK(c, s->A.ensure(sizeof(double) * bel * P));
  HIPCHK(c, s->alpha.ensure(sizeof(double) * (size_t)m.np * P));
  HIPCHK(c, s->partial.ensure(sizeof(double) * 2 * (size_t)P));
  HIPCHK(c, s->out_lp.ensure(sizeof(double) * (size_t)P + sizeof(int32_t) * (size_t)P));
  HIPCHK(c, hipMemcpyAsync(s->dense.p, K, sizeof(double) * nel * P, hipMemcpyHostToDevice, st));
  if (y) HIPCHK(c, hipMemcpyAsync(s->vec.p, y, sizeof(double) * (size_t)n * P, hipMemcpyHostToDevice, st));
  SeriesProbeArgs sa = {};
  sa.K = s->dense.as<double>(); sa.y = y ? s->vec.as<double>() : nullptr; sa.n = (int)n;
  sa.out_blk = s->A.as<double>(); sa.out_alpha = s->alpha.as<double>(); sa.out_part = s->partial.as<double>();
  sa.out_lp = s->out_lp.as<double>(); sa.out_info = reinterpret_cast<int32_t*>(s->out_lp.as<double>() + P);
  HIPCHK(c, launch_series_probe(st, sa, P, sizeof(double) * (size_t)m.total));
  std::vector<double> blk(bel * P), av((size_t)m.np * P);
  HIPCHK(c, hipMemcpyAsync(blk.data(), s->A.p, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(av.data(), s->alpha.p, sizeof(double) * av.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_part, s->partial.p, sizeof(double) * 2 * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_lp, s->out_lp.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_info, sa.out_info, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  // element (r, col) of block (rb, cb) sits at col * 16 + r of block rb (rb + 1) / 2 + cb (blk_idx): row-major L, zeros above the diagonal
  for (int p = 0; p < P; ++p) {
    const double* b = blk.data() + (size_t)p * bel;
    double* L = out_L + (size_t)p * nel;
    for (int64_t r = 0; r < n; ++r)
      for (int64_t col = 0; col < n; ++col) {
        const size_t at = ((size_t)(r / 16) * (r / 16 + 1) / 2 + (size_t)(col / 16)) * 256 + (size_t)(col % 16) * 16 + (size_t)(r % 16);
        L[r * n + col] = col <= r ? b[at] : 0.0;
      }
    std::copy(av.begin() + (size_t)p * m.np, av.begin() + (size_t)p * m.np + n, out_alpha + (size_t)p * n);
  }
  return AGP_OK;
}

}  // namespace

extern "C" {

int agp_logpdf_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P,
                            const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                            const double* noise, double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&] { return series_batch(c, S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, nullptr}, series, out_logpdf, out_info); });
}

int agp_logpdf_grad_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P,
                                 const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                 const double* noise, double* out_logpdf, double* out_grad, double* out_grad_noise, int32_t* out_info) {
  return abi_guard(c, [&] {
    const GradOut go{out_grad, out_grad_noise};
    return series_batch(c, S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, nullptr}, series, out_logpdf, out_info, &go);
  });
}

int agp_predict_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, const int64_t* q_off,
                             const double* ts_pred, int32_t P, const int32_t* series, const int32_t* op_off, const uint8_t* ops,
                             const int32_t* prm_off, const double* prm, const double* noise, const double* noise_pred, double* out_mean,
                             double* out_var, int64_t* out_off, double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&] {
    const SeriesPredOut po{q_off, ts_pred, out_mean, out_var, out_off};
    return series_batch(c, S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, out_logpdf, out_info, nullptr, &po);
  });
}

int agp_predict_quantile_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs,
                                      const int64_t* q_off, const double* ts_pred, int32_t P, const int32_t* series, const int32_t* op_off,
                                      const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                                      const double* noise_pred, const double* weights, const double* y_slope, const double* y_intercept,
                                      const double* q, int64_t nq, double tol, int64_t max_iter, double* out_x, int32_t* out_converged,
                                      int32_t* out_iters, double* out_mix_mean, double* out_mix_var, double* out_logpdf,
                                      int32_t* out_info) {
  return abi_guard(c, [&] {
    const SeriesPredOut po{q_off, ts_pred, nullptr, nullptr, nullptr};
    const SeriesQuantOut qo{weights, y_slope, y_intercept, q, nq, tol, max_iter, out_x, out_converged, out_iters, out_mix_mean, out_mix_var};
    return series_batch(c, S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, out_logpdf, out_info, nullptr, &po,
                        &qo);
  });
}

int agp_debug_series_factor(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, double* out_L, double* out_alpha,
                            double* out_partial, double* out_lp, int32_t* out_info) {
  return abi_guard(c, [&] { return series_factor(c, K, y, n, P, out_L, out_alpha, out_partial, out_lp, out_info); });
}

}  // extern "C"
