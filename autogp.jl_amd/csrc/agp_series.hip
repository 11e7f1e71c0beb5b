// The many-series entries: many SHORT series, each with its own particles, in one call of the small-matrix kernels
// (agp_series_kernel.hpp: one workgroup per particle, covariance + Cholesky + forward solve + value in LDS).
//   agp_logpdf_series_batch            k_series_logpdf: the values
//   agp_logpdf_long_series_batch       the same values for series of up to AGP_LONG_SERIES_MAX_N points: k_series_logpdf up to the short
//                                      cap, k_long_series_logpdf (agp_long_series_kernel.hpp: the factor in an HBM workspace) above it
//   agp_logpdf_grad_series_batch       k_series_logpdf_grad: L^-T, alpha and the contraction with dK / d theta behind the value
//   agp_hmc_series_batch               k_series_hmc: the gradient kernel's statements in a loop — HMC moves of every particle's parameters
//                                      and noise in the reference's latent space, the whole chain of a particle in one workgroup
//   agp_predict_series_batch           k_series_predict: posterior mean and marginal variance at every series' own query times
//   agp_predict_long_series_batch      the same forecast for series of up to AGP_LONG_SERIES_MAX_N points: k_series_predict up to the short
//                                      cap, k_long_series_predict above it; agp_predict_quantile_long_series_batch: its band
//   agp_predict_quantile_series_batch  the predictive launches, their device outputs read out by agp_series_quantile_kernel.hpp on
//                                      the same stream: quantiles and marginal moments of every series' own mixture
//   agp_predict_logpdf_series_batch    k_series_predict_logpdf: the value kernel on the joint points, the query rows' partials read out —
//                                      the log-density of every series' held-out values; k_series_mix_logp behind it for the mixtures
//   agp_predict_logpdf_long_series_batch  the same scores for n_s + m_s up to AGP_LONG_SERIES_MAX_N joint points: k_series_predict_logpdf
//                                      up to the short cap, k_long_series_predict_logpdf above it; the same mixture read-out
//   agp_predict_sample_series_batch    k_series_predict_sample: the same joint factorisation with a zero query right-hand side, the query
//                                      rows read out as samples, component means and covariances; k_series_sample_fill behind it
//   agp_predict_sum_series_batch       k_series_predict_sum: the predictive kernel on every particle's composite program (append_composite)
//                                      and coded query rows F_1 .. F_M, X, read out as predict_sum's raw marginals and quantiles
// Each entry is one function, read top to bottom, over the stages they share (one SeriesCall carries what a stage leaves for the next):
//   checks          series_check_sizes, series_check_pointers, series_check_layout (the entry's own pointer checks between them)
//   series_classes  compile, per particle length / LDS need / evaluation stack, launch classes, workgroup order, out_off
//   series_stage    the slot, its buffers and the uploads every mode needs (and the query side when there are queries), SeriesArgs;
//                   behind it series_query_args (the query side of a kernel's arguments), series_grad_tape (the gradient tape: buffers,
//                   uploads, SeriesGradArgs) and series_stage_mix (a mixture plan's tables in sq_tab)
//   series_launch   the class x LDS-class loop, between the profiling events; the entry passes what launches one class
//   series_fetch / series_copy_values   [logpdf | info] and every device array the entry registered (SeriesCall::want) into the
//                   pinned landing zone, the stream drained; the values out of it (the entry's own arrays: SeriesCall::got)
//   series_timing   agp_get_timing's slots (the read-out span when the entry marked one: series_mark_readout)
// What a series' mixture needs — the particle lists, the checked and padded weights — is one plan (mix_plan) for the band, the held-out
// and the sampling entry; what is refused series by series (series_check_joint, series_y_transform) is called from each entry's own
// loop over the series, so that the lowest series with a defect is the one reported.  An entry still owns: its pointer checks, its
// planning, its buffers and uploads, its kernel's arguments, what it registers for read-back, and the copy-out.  ONE
// PinnedUploads::flush and ONE hipStreamSynchronize per call.  Stateless: the series
// travel with the call; the resident series, its tables, the factor store, the coalescer and every counter of the context are
// neither read nor changed — only a workspace slot (stream, staging buffers) is borrowed, as in every batch entry.
#include "agp_host.hpp"
#include "agp_ndtri.hpp"

#include <optional>

static_assert(SERIES_MAX_N == AGP_SERIES_MAX_N, "the kernel's cap is the C ABI's");
static_assert(AGP_SERIES_MAX_N >= 160, "the reference's 126-, 135-, 143- and 144-point series must fit");
static_assert(LONG_SERIES_MAX_N == AGP_LONG_SERIES_MAX_N, "the long kernel's cap is the C ABI's");
static_assert(AGP_LONG_SERIES_MAX_N >= 442 && AGP_LONG_SERIES_MAX_N > AGP_SERIES_MAX_N, "the reference's 442-point series must fit");

namespace {

// LDS classes of the launches: a launch declares the largest need of its particles, so particles are grouped by how many workgroups
// of their size share a CU's 160 KiB — 4 (n <= ~80), 2 (n <= ~128) or 1.
int lds_class(size_t bytes) { return bytes <= (size_t)SERIES_LDS_BYTES / 4 ? 0 : bytes <= (size_t)SERIES_LDS_BYTES / 2 ? 1 : 2; }

// The band of agp_predict_quantile_series_batch: the mixtures' weights and transforms, the quantiles, and the outputs (host).
struct SeriesQuantOut {
  const double* weights;     // [P] particle p's weight inside its series' mixture
  const double* y_slope;     // [S] or null (1)
  const double* y_intercept; // [S] or null (0)
  const double* q; int64_t nq; double tol; int64_t max_iter;
  double* x; int32_t* conv; int32_t* iters;      // [nq q_off[S]]; conv / iters nullable
  double* mix_mean; double* mix_var;              // [q_off[S]], nullable
};

// The mixtures of a call's series — what the read-out kernels index with, built and checked on the host before anything is launched
// or written: the band's, the held-out and the sampling entry's.
struct MixPlan {
  std::vector<long long> tab;      // [pl_off (S + 1) | w_off (S + 1) | row_off (S + 1)]
  std::vector<int32_t> plist;      // [P] the series' particles, series by series, ascending within each
  std::vector<double> vals;        // [w (w_off[S], 0 in the padding) | slope (S) | intercept (S)]; the band adds [ivar (S) | q (nq)]
  long long max_rows_el = 0;       // largest m_s Pp_s
  size_t Q = 0, R = 0, W = 0;      // q_off[S], row_off[S], w_off[S]
  const long long* pl_off() const { return tab.data(); }
  const long long* w_off() const { return tab.data() + tab.size() / 3; }
};

// prefixes the message a shared check has just stored with the series it was about
int fail_series(agp_ctx* c, int rc, int32_t s) {
  std::string msg;
  { std::lock_guard<std::mutex> g(c->mu); msg = c->err; }
  return fail(c, rc, "series " + std::to_string(s) + ": " + msg);
}

// series s' (slope, intercept) — 1 and 0 where the caller gave none — checked; a refusal names the series
int series_y_transform(agp_ctx* c, int32_t s, const double* y_slope, const double* y_intercept, double& slope, double& icpt) {
  slope = y_slope ? y_slope[s] : 1.0;
  icpt = y_intercept ? y_intercept[s] : 0.0;
  const int rc = check_y_transform(c, slope, icpt);
  return rc ? fail_series(c, rc, s) : AGP_OK;
}

// The mixture plan.  nq: outputs per query point (the band's quantiles; 0 elsewhere), for the limit on the largest output.
// y_slope / y_intercept: the band's transforms, checked series by series in one pass with the weights — the lowest series with a
// defect of either kind is the one refused (the other entries have checked theirs in their own loop, and pass none).  The limits
// on w_off and on row_off — the band's rows m_s ceil(P_s / 64) 64, which only the band reads — hold for every caller: the
// held-out and the sampling entry have always refused what the band refuses here, and go on doing so.
int mix_plan(agp_ctx* c, int32_t S, int P, const int32_t* series, const int64_t* q_off, const double* weights, const double* y_slope,
             const double* y_intercept, int64_t nq, MixPlan& pl) {
  if (!weights && P > 0) return fail(c, AGP_ERR_ARG, "null weights");
  pl.Q = S > 0 ? (size_t)q_off[S] : 0;
  if ((int64_t)pl.Q >= ((int64_t)1 << 31) || (nq > 0 && (int64_t)pl.Q * nq >= ((int64_t)1 << 31)))
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
  pl.vals.assign(pl.W + 2 * (size_t)S, 0.0);
  double* w = pl.vals.data();
  double* slope = w + pl.W;
  double* icpt = slope + S;
  std::vector<double> ws;
  for (int32_t s = 0; s < S; ++s) {
    if (const int rc = series_y_transform(c, s, y_slope, y_intercept, slope[s], icpt[s])) return rc;
    const long long Ps = pl_off[s + 1] - pl_off[s];
    if (Ps == 0) continue;
    ws.resize((size_t)Ps);
    for (long long j = 0; j < Ps; ++j) ws[(size_t)j] = weights[pl.plist[(size_t)(pl_off[s] + j)]];
    if (const int rc = check_weights(c, (int32_t)Ps, ws.data())) return fail_series(c, rc, s);
    std::copy(ws.begin(), ws.end(), w + w_off[s]);
  }
  return AGP_OK;
}

// The band's plan: its own checks, its mixtures', and behind the plan's values its own — vals = [.. | ivar (S) | q (nq)]
int quant_plan(agp_ctx* c, int32_t S, int P, const int32_t* series, const int64_t* q_off, const SeriesQuantOut& qo, MixPlan& pl) {
  if (qo.nq < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (!qo.q && qo.nq > 0) return fail(c, AGP_ERR_ARG, "null q");
  for (int64_t k = 0; k < qo.nq; ++k)
    if (!(qo.q[k] > 0.0 && qo.q[k] < 1.0)) return fail(c, AGP_ERR_ARG, "quantile must be in (0, 1)");
  if (!qo.x && qo.nq > 0) return fail(c, AGP_ERR_ARG, "null pointer argument (out_x)");
  if (const int rc = mix_plan(c, S, P, series, q_off, qo.weights, qo.y_slope, qo.y_intercept, qo.nq, pl)) return rc;
  const size_t o_ivar = pl.vals.size();
  pl.vals.resize(o_ivar + (size_t)S + (size_t)qo.nq);
  for (int32_t s = 0; s < S; ++s) pl.vals[o_ivar + s] = 1.0 / (pl.vals[pl.W + s] * pl.vals[pl.W + s]);
  std::copy(qo.q, qo.q + qo.nq, pl.vals.data() + o_ivar + (size_t)S);
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

#define STAGE(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

// Which kernel the call launches: it chooses the LDS map, the instantiation rule and (gradient) the tape's limit.
// long_value: the value entry for series of up to AGP_LONG_SERIES_MAX_N points — a particle above the short cap (or every particle,
// SeriesCall::all_long) takes k_long_series_logpdf and its map, the others are the value mode's.
// long_prediction: the same routing for the forecast and the band — k_long_series_predict and its map above the short cap, the
// prediction mode's kernel and map below it.
// long_held_out: the same routing by the JOINT length n_s + m_s for the held-out scores — k_long_series_predict_logpdf on the long
// value kernel's map and workspace above the short cap, the held-out mode's kernel and map below it.
enum class SeriesMode { value, gradient, prediction, held_out, sum, hmc, long_value, long_prediction, long_held_out };
constexpr int SERIES_LONG_CLASS = 3;      // launch classes 3, 4: the long kernel<4 / 8> of the mode (0 .. 2: the mode's short kernels)

// One call of a many-series entry: the caller's inputs and what each shared stage leaves for the later ones.
struct SeriesCall {
  // inputs (q_off / ts_pred: null in the entries without queries)
  int32_t S; const int64_t* pt_off; const double* ts; const double* xs; Particles pp; const int32_t* series;
  const int64_t* q_off; const double* ts_pred;
  int hmc_C = 0;                     // HMC entry: transform classes (the LDS map holds their table)
  int max_n = AGP_SERIES_MAX_N;      // the entry's cap on a series' length, and the name the refusal quotes
  const char* max_name = "AGP_SERIES_MAX_N";
  bool all_long = false;             // long entry: every non-empty series takes the long kernel (AGP_LONG_SERIES_ALL)
  bool long_route(int n) const { return n > SERIES_MAX_N || (all_long && n > 0); }
  long long (*ws_blocks)(int) = long_series_ws_blocks;      // long entries: workspace blocks of a workgroup with nb block rows
  // series_classes
  Batch bt;                          // programs without any table of the resident series (no log|dt| table, no lag tables), caller's order
  std::vector<int> len;              // [P] points of the particle's series
  std::vector<size_t> need;          // [P] LDS bytes
  std::vector<int64_t> nq;           // [P] query points of the particle's series (0 without queries)
  std::vector<int32_t> list[5][3];   // launch classes (kernel instantiation) x (LDS class), longest series first inside each
  std::vector<int32_t> wg;           // ... one behind the other in launch order; empty: nothing to launch
  std::vector<long long> ooff;       // [P + 1] with queries: out_off, the particle-major layout of the prediction
  // series_stage
  std::optional<SlotGuard> sg;
  Slot* s = nullptr; hipStream_t st = nullptr;
  size_t npts = 0, nqt = 0;          // pt_off[S], q_off[S]; tt = [ts | xs | ts_pred]
  size_t o_series = 0, o_wg = 0, o_qoff = 0, o_ooff = 0;      // bytes; map = [pt_off (int64) | series | wg | q_off (int64) | out_off (int64)]
  PinnedUploads up;                  // the call's one upload: the stage's arrays, then the entry's own
  SeriesArgs sa = {};                // all but wg, which every launch sets
  // series_launch
  bool prof = false; hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  bool readout = false;              // ev[2] was recorded behind the entry's read-out kernels (series_mark_readout)
  int64_t ws_limit = 0;              // series_long_workspace: the bytes one long launch's workspace may take
  bool ws_used = false;              // series_launch_long: a long launch of this call has used the workspace
  size_t n_out() const { return ooff.empty() ? 0 : (size_t)ooff.back(); }
  size_t values_bytes() const { return sizeof(double) * (size_t)pp.P + sizeof(int32_t) * (size_t)pp.P; }
  template <class T> T* in_map(size_t off) const { return reinterpret_cast<T*>(s->map.as<char>() + off); }
  // series_fetch: the read-back list, PinnedUploads' mirror image.  The pinned landing zone begins with [logpdf (P) | info (P)];
  // the device arrays the entry wants back follow in the order it asked for them, each at a multiple of 8 bytes
  struct Back { const void* dev; size_t bytes, off; };
  std::vector<Back> back;
  int want(const void* dev, size_t bytes) { back.push_back({dev, bytes, 0}); return (int)back.size() - 1; }
  template <class T> const T* got(int h) const { return reinterpret_cast<const T*>(static_cast<const char*>(s->h_out.p) + back[(size_t)h].off); }
};

// The checks, in this order, the entry's own pointer checks between the second and the third.
int series_check_sizes(agp_ctx* c, const SeriesCall& sc) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  return sc.S < 0 || sc.pp.P < 0 ? fail(c, AGP_ERR_ARG, "negative number of series or particles") : AGP_OK;
}
// outputs: the value outputs this entry cannot do without are there
int series_check_pointers(agp_ctx* c, const SeriesCall& sc, bool outputs) {
  const bool ok = sc.pt_off && sc.ts && sc.xs && sc.series && sc.pp.complete() && outputs;
  return ok ? AGP_OK : fail(c, AGP_ERR_ARG, "null pointer argument");
}

int series_check_layout(agp_ctx* c, const SeriesCall& sc) {
  const int32_t S = sc.S;
  const int64_t* pt_off = sc.pt_off;
  char buf[256];
  if (S > 0 && pt_off[0] != 0) return fail(c, AGP_ERR_ARG, "pt_off[0] must be 0 (series 0)");
  for (int32_t s = 0; s < S; ++s) {
    if (pt_off[s + 1] < pt_off[s]) {
      snprintf(buf, sizeof buf, "series %d: pt_off decreases (%lld after %lld)", (int)s, (long long)pt_off[s + 1], (long long)pt_off[s]);
      return fail(c, AGP_ERR_ARG, buf);
    }
    if (pt_off[s + 1] - pt_off[s] > sc.max_n) {
      snprintf(buf, sizeof buf, "series %d has %lld points, more than %s (%d)", (int)s, (long long)(pt_off[s + 1] - pt_off[s]),
               sc.max_name, sc.max_n);
      return fail(c, AGP_ERR_ARG, buf);
    }
  }
  if (const int64_t* q_off = sc.q_off) {
    if (S > 0 && q_off[0] != 0) return fail(c, AGP_ERR_ARG, "q_off[0] must be 0 (series 0)");
    for (int32_t s = 0; s < S; ++s) {
      if (q_off[s + 1] < q_off[s]) {
        snprintf(buf, sizeof buf, "series %d: q_off decreases (%lld after %lld)", (int)s, (long long)q_off[s + 1], (long long)q_off[s]);
        return fail(c, AGP_ERR_ARG, buf);
      }
      if (q_off[s + 1] - q_off[s] > (int64_t)1 << 30) {
        snprintf(buf, sizeof buf, "series %d has %lld query points, more than 2^30", (int)s, (long long)(q_off[s + 1] - q_off[s]));
        return fail(c, AGP_ERR_ARG, buf);
      }
    }
  }
  for (int p = 0; p < sc.pp.P; ++p)
    if (sc.series[p] < 0 || sc.series[p] >= S) {
      snprintf(buf, sizeof buf, "particle %d: series index %d outside [0, %d)", p, (int)sc.series[p], (int)S);
      return fail(c, AGP_ERR_ARG, buf);
    }
  for (int p = 0; p < sc.pp.P; ++p)
    if (sc.pp.op_off[p] < 0 || sc.pp.prm_off[p] < 0 || sc.pp.op_off[p + 1] < sc.pp.op_off[p] || sc.pp.prm_off[p + 1] < sc.pp.prm_off[p]) {
      snprintf(buf, sizeof buf, "particle %d: malformed program / parameter offsets", p);
      return fail(c, AGP_ERR_ARG, buf);
    }
  return AGP_OK;
}

// the entries that factor a series' training and query points together (what: "held-out" or "query"): the joint size of series s
// against the entry's cap (max_n, named max_name: the short entries' AGP_SERIES_MAX_N, the long held-out entry's AGP_LONG_SERIES_MAX_N)
int series_check_joint(agp_ctx* c, const SeriesCall& sc, int32_t s, const char* what, int max_n = AGP_SERIES_MAX_N,
                       const char* max_name = "AGP_SERIES_MAX_N") {
  const long long n = sc.pt_off[s + 1] - sc.pt_off[s], m = sc.q_off[s + 1] - sc.q_off[s];
  if (m == 0 || n + m <= max_n) return AGP_OK;
  char buf[256];
  snprintf(buf, sizeof buf, "series %d has %lld training and %lld %s points, together more than %s (%d)", (int)s, n, m, what, max_name,
           max_n);
  return fail(c, AGP_ERR_ARG, buf);
}

// LDS bytes of particle p on a series of n points (held_out — the held-out and the sampling entry —: the joint n_s + m_s points, the
// value kernel's map; long_held_out: the joint points as well, the long value kernel's map on the long route): the mode's own map
size_t series_need(SeriesMode mode, const Batch& bt, int p, int n, int hmc_C = 0, bool long_route = false) {
  const ProgHdr& h = bt.hdr[(size_t)p];
  const bool long_pred = mode == SeriesMode::long_prediction;
  if (long_pred && !long_route) mode = SeriesMode::prediction;      // (below the short cap: the prediction mode's kernel and map)
  const int m_total = long_route ? (long_pred ? long_series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp).total
                                               : long_series_lds(n, h.n_ops, h.n_prm, h.n_cp).total)
                      : mode == SeriesMode::hmc ? series_hmc_lds(n, h.n_ops, h.n_prm, h.n_cp, bt.ghdr[(size_t)p].n_ops, bt.ghdr[(size_t)p].n_prm, hmc_C).total
                      : mode == SeriesMode::gradient ? series_grad_lds(n, h.n_ops, h.n_prm, h.n_cp, bt.ghdr[(size_t)p].n_ops, bt.ghdr[(size_t)p].n_prm).total
                      : mode == SeriesMode::prediction || mode == SeriesMode::sum ? series_pred_lds(n, h.n_ops, h.n_prm, h.n_cp).total
                                                       : series_lds(n, h.n_ops, h.n_prm, h.n_cp).total;
  return sizeof(double) * (size_t)m_total;
}

// the evaluation stack one program needs (compile_batch reports the batch's largest only): from the compiled postfix form
int series_stack_depth(const Batch& bt, const ProgHdr& h) {
  int sp = 0, depth = 0;
  for (int i = 0; i < h.n_ops; ++i) {
    const int o = bt.ops[(size_t)h.op_off + i];
    if (o == OP_PLUS || o == OP_TIMES || o == OP_CP || o == OP_CP_SWAP) --sp; else ++sp;
    depth = std::max(depth, sp);
  }
  return depth;
}

// compile; per particle: length, LDS need, instantiation; launch classes, longest series first inside each; wg and out_off.
// Instantiations: values and predictions — evaluation-stack depth 4 / 8; gradient — tape of 16 / 64 nodes, the 64-node tape with the
// depth the value entry picks for the same program (<= 16 nodes never need more than 4), so that the value's bits are that entry's
int series_classes(agp_ctx* c, SeriesCall& sc, SeriesMode mode) {
  const int P = sc.pp.P;
  char buf[256];
  Batch& bt = sc.bt;
  CompileOpts co;
  co.ge_tab = false; co.lag = false; co.never_fuse = true; co.want_grad = mode == SeriesMode::gradient || mode == SeriesMode::hmc;
  co.allow_sel = mode == SeriesMode::sum;      // (the composite programs' selector leaves: one per-point table each, counted in n_cp)
  STAGE(compile_batch(c, sc.pp, bt, co));
  const bool grad_mode = mode == SeriesMode::gradient || mode == SeriesMode::hmc;      // (the HMC kernel is the gradient kernel in a loop)
  if (grad_mode)
    for (int p = 0; p < P; ++p)
      if (bt.ghdr[(size_t)p].n_ops > 64) {      // (RegTape<64> is the largest tape: agp_logpdf_grad_batch's own limit)
        snprintf(buf, sizeof buf, "particle %d: gradient supports kernel trees of up to 64 nodes (%d)", p, (int)bt.ghdr[(size_t)p].n_ops);
        return fail(c, AGP_ERR_PROGRAM, buf);
      }
  sc.len.assign((size_t)P, 0);
  sc.need.assign((size_t)P, 0);
  sc.nq.assign((size_t)P, 0);
  for (int p = 0; p < P; ++p) {
    if (bt.order[(size_t)p] != p) return fail(c, AGP_ERR_HOST, "internal error: compiled batch out of order");
    const ProgHdr& h = bt.hdr[(size_t)p];
    const int32_t s = sc.series[p];
    int n = (int)(sc.pt_off[s + 1] - sc.pt_off[s]);
    sc.len[(size_t)p] = n;
    if (sc.q_off) sc.nq[(size_t)p] = sc.q_off[s + 1] - sc.q_off[s];
    // held-out scores: the workgroup factors the JOINT points, so length, LDS need, class and "longest first" are those of
    // n_s + m_s; nothing held out scores 0 without a launch, as an empty series does in the value entry
    if (mode == SeriesMode::held_out || mode == SeriesMode::long_held_out)
      sc.len[(size_t)p] = n = sc.nq[(size_t)p] > 0 ? n + (int)sc.nq[(size_t)p] : 0;
    if (n == 0 && sc.nq[(size_t)p] == 0) continue;      // (an empty series is launched for its prior predictive only)
    const bool lng = (mode == SeriesMode::long_value || mode == SeriesMode::long_prediction || mode == SeriesMode::long_held_out) &&
                     sc.long_route(n);
    const size_t need = sc.need[(size_t)p] = series_need(mode, bt, p, n, sc.hmc_C, lng);
    if (need > (size_t)SERIES_LDS_BYTES) {
      snprintf(buf, sizeof buf, "particle %d: %d per-point tables (%s) at %d points need %zu bytes of LDS, more than the "
               "kernel's %d", p, (int)h.n_cp, mode == SeriesMode::sum ? "ChangePoint nodes and component selectors" : "ChangePoint nodes", n,
               need, SERIES_LDS_BYTES);
      return fail(c, AGP_ERR_PROGRAM, buf);
    }
    const int depth = series_stack_depth(bt, h);
    const int inst = !grad_mode ? (depth <= 4 ? 0 : 1) : bt.ghdr[(size_t)p].n_ops <= 16 && depth <= 4 ? 0 : depth <= 4 ? 1 : 2;
    sc.list[lng ? SERIES_LONG_CLASS + inst : inst][lds_class(need)].push_back(p);
  }
  for (auto& ld : sc.list)
    for (auto& v : ld) std::stable_sort(v.begin(), v.end(), [&](int32_t x, int32_t y) { return sc.len[(size_t)x] > sc.len[(size_t)y]; });
  sc.wg.reserve((size_t)P);
  for (auto& ld : sc.list) for (auto& v : ld) sc.wg.insert(sc.wg.end(), v.begin(), v.end());
  if (sc.q_off) {
    sc.ooff.assign((size_t)P + 1, 0);
    for (int p = 0; p < P; ++p) sc.ooff[(size_t)p + 1] = sc.ooff[(size_t)p] + sc.nq[(size_t)p];
  }
  return AGP_OK;
}

// what every entry writes when no particle is launched: every particle scores an empty series (src/inference_smc_anneal_data.jl:185-187)
// and has nothing to predict
void series_zero_values(const SeriesCall& sc, double* out_logpdf, int32_t* out_info) {
  if (out_logpdf) std::fill(out_logpdf, out_logpdf + sc.pp.P, 0.0);
  std::fill(out_info, out_info + sc.pp.P, 0);
}

// The slot, its stream, and the device buffers and uploads every mode uses: programs as in every sweep; tt = [ts | xs];
// map = [pt_off (int64) | series | wg]; the values in out_lp = [logpdf | info].  With queries: tt = [ts | xs | ts_pred];
// map = [.. | q_off (int64) | out_off (int64)]; noise_pred (null: the particle's own noise); the outputs in pred_mean / pred_var.
// Fills sc.sa; the entry adds its own uploads to sc.up and flushes it.
int series_stage(agp_ctx* c, SeriesCall& sc) {
  const int P = sc.pp.P;
  const size_t S1 = (size_t)sc.S + 1;
  const Batch& bt = sc.bt;
  HIPCHK(c, hipSetDevice(c->device));
  sc.sg.emplace(c);
  Slot* s = sc.s = sc.sg->s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  sc.st = s->stream;
  const size_t npts = sc.npts = (size_t)sc.pt_off[sc.S];
  sc.nqt = sc.q_off ? (size_t)sc.q_off[sc.S] : 0;
  sc.o_series = sizeof(long long) * S1;
  sc.o_wg = sc.o_series + sizeof(int32_t) * (size_t)P;
  sc.o_qoff = (sc.o_wg + sizeof(int32_t) * sc.wg.size() + 7) & ~(size_t)7;
  sc.o_ooff = sc.o_qoff + sizeof(long long) * S1;
  HIPCHK(c, s->hdr.ensure(sizeof(ProgHdr) * (size_t)P));
  HIPCHK(c, s->ops.ensure(bt.ops.size() + 4));
  HIPCHK(c, s->prm.ensure(sizeof(double) * std::max<size_t>(1, bt.prm.size())));
  HIPCHK(c, s->noise.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->tt.ensure(sizeof(double) * 2 * std::max<size_t>(1, npts)));
  HIPCHK(c, s->map.ensure(sc.o_wg + sizeof(int32_t) * sc.wg.size()));
  HIPCHK(c, s->out_lp.ensure(sc.values_bytes()));
  if (sc.q_off) {
    HIPCHK(c, s->tt.ensure(sizeof(double) * (2 * std::max<size_t>(1, npts) + std::max<size_t>(1, sc.nqt))));
    HIPCHK(c, s->map.ensure(sc.o_ooff + sizeof(long long) * ((size_t)P + 1)));
    HIPCHK(c, s->noise_pred.ensure(sizeof(double) * (size_t)P));
    HIPCHK(c, s->pred_mean.ensure(sizeof(double) * std::max<size_t>(1, sc.n_out())));
    HIPCHK(c, s->pred_var.ensure(sizeof(double) * std::max<size_t>(1, sc.n_out())));
  }
  const std::vector<long long> off64(sc.pt_off, sc.pt_off + S1);
  PinnedUploads& up = sc.up;
  up.add(s->hdr.p, bt.hdr.data(), sizeof(ProgHdr) * (size_t)P);
  up.add(s->ops.p, bt.ops.data(), bt.ops.size());
  up.add(s->prm.p, bt.prm.data(), sizeof(double) * bt.prm.size());
  up.add(s->noise.p, sc.pp.noise, sizeof(double) * (size_t)P);
  up.add(s->tt.p, sc.ts, sizeof(double) * npts);
  up.add(s->tt.as<double>() + npts, sc.xs, sizeof(double) * npts);
  up.add(s->map.p, off64.data(), sc.o_series);
  up.add(sc.in_map<char>(sc.o_series), sc.series, sizeof(int32_t) * (size_t)P);
  up.add(sc.in_map<char>(sc.o_wg), sc.wg.data(), sizeof(int32_t) * sc.wg.size());
  if (sc.q_off) {
    const std::vector<long long> qoff64(sc.q_off, sc.q_off + S1);
    up.add(sc.in_map<char>(sc.o_qoff), qoff64.data(), sizeof(long long) * S1);
    up.add(sc.in_map<char>(sc.o_ooff), sc.ooff.data(), sizeof(long long) * ((size_t)P + 1));
    up.add(s->tt.as<double>() + 2 * npts, sc.ts_pred, sizeof(double) * sc.nqt);
    up.add(s->noise_pred.p, sc.pp.noise_pred ? sc.pp.noise_pred : sc.pp.noise, sizeof(double) * (size_t)P);
  }
  SeriesArgs& sa = sc.sa;
  sa.ts = s->tt.as<double>(); sa.xs = s->tt.as<double>() + npts;
  sa.pt_off = s->map.as<long long>();
  sa.series = sc.in_map<const int32_t>(sc.o_series);
  sa.hdr = s->hdr.as<ProgHdr>(); sa.ops = s->ops.as<uint8_t>(); sa.prm = s->prm.as<double>(); sa.noise = s->noise.as<double>();
  sa.out_lp = s->out_lp.as<double>(); sa.out_info = reinterpret_cast<int32_t*>(s->out_lp.as<double>() + P);
  return AGP_OK;
}

// a kernel's arguments of a staged call with queries: the SeriesArgs base and the query side
template <class Args> void series_query_args(const SeriesCall& sc, Args& a) {
  static_cast<SeriesArgs&>(a) = sc.sa;
  a.q_off = sc.in_map<const long long>(sc.o_qoff);
  a.out_off = sc.in_map<const long long>(sc.o_ooff);
  a.ts_pred = sc.s->tt.as<double>() + 2 * sc.npts; a.noise_pred = sc.s->noise_pred.as<double>();
}

// the gradient tape of a staged call: its buffers, its uploads (into sc.up), and the arguments that name it — all of ga but the
// gradient's outputs, which are the entry's own
int series_grad_tape(agp_ctx* c, SeriesCall& sc, SeriesGradArgs& ga) {
  Slot* s = sc.s;
  const Batch& bt = sc.bt;
  const size_t P = (size_t)sc.pp.P;
  const struct { DevBuf& buf; const void* src; size_t bytes, slack; } parts[] = {      // (slack: bytes of the buffer behind the upload)
      {s->ghdr, bt.ghdr.data(), sizeof(GProgHdr) * P, 0},
      {s->gops, bt.gops.data(), bt.gops.size(), 4},
      {s->glc, bt.glc.data(), bt.glc.size(), 4},
      {s->grc, bt.grc.data(), bt.grc.size(), 4},
      {s->gpoff, bt.gpoff.data(), sizeof(int32_t) * bt.gpoff.size(), sizeof(int32_t)},
      {s->gprm, bt.gprm.data(), sizeof(double) * bt.gprm.size(), 0},
      {s->gmap, bt.gmap.data(), sizeof(int32_t) * bt.gmap.size(), sizeof(int32_t)},
      {s->goff, sc.pp.prm_off, sizeof(int32_t) * P, 0}};      // the particle's block in out_grad: the caller's own offsets
  for (const auto& t : parts) {
    HIPCHK(c, t.buf.ensure(t.bytes + t.slack));
    sc.up.add(t.buf.p, t.src, t.bytes);
  }
  static_cast<SeriesArgs&>(ga) = sc.sa;
  ga.ghdr = s->ghdr.as<GProgHdr>(); ga.gops = s->gops.as<uint8_t>(); ga.glc = s->glc.as<uint8_t>(); ga.grc = s->grc.as<uint8_t>();
  ga.gpoff = s->gpoff.as<int32_t>(); ga.gprm = s->gprm.as<double>(); ga.gmap = s->gmap.as<int32_t>();
  ga.out_off = s->goff.as<int32_t>();
  return AGP_OK;
}

// a mixture plan's tables of a staged call: sq_tab = [pl_off | w_off | row_off (S + 1 each) | plist (P)], uploaded through sc.up
struct MixTabs { const long long* pl_off; const long long* w_off; const long long* row_off; const int32_t* plist; };
int series_stage_mix(agp_ctx* c, SeriesCall& sc, const MixPlan& mp, MixTabs& mt) {
  Slot* s = sc.s;
  const size_t S1 = (size_t)sc.S + 1, o_plist = sizeof(long long) * 3 * S1;
  HIPCHK(c, s->sq_tab.ensure(o_plist + sizeof(int32_t) * (size_t)sc.pp.P));
  sc.up.add(s->sq_tab.p, mp.tab.data(), o_plist);
  sc.up.add(s->sq_tab.as<char>() + o_plist, mp.plist.data(), sizeof(int32_t) * (size_t)sc.pp.P);
  mt.pl_off = s->sq_tab.as<long long>(); mt.w_off = mt.pl_off + S1; mt.row_off = mt.w_off + S1;
  mt.plist = reinterpret_cast<const int32_t*>(s->sq_tab.as<char>() + o_plist);
  return AGP_OK;
}

// The classes in order, between the first two profiling events.  launch(wg, grid, d, lds_bytes) -> hipError_t launches the `grid`
// particles wg[0 .. grid) of instantiation class d with the largest LDS need among them (d >= SERIES_LONG_CLASS: the long entry's alone).
template <class Launch> int series_launch(agp_ctx* c, SeriesCall& sc, Launch&& launch) {
  Slot* s = sc.s;
  sc.prof = c->profiling;
  if (sc.prof) {
    while (s->events.size() < 3) { hipEvent_t e; HIPCHK(c, hipEventCreate(&e)); s->events.push_back(e); }
    sc.ev[0] = s->events[0]; sc.ev[1] = s->events[1]; sc.ev[2] = s->events[2];
    HIPCHK(c, hipEventRecord(sc.ev[0], sc.st));
  }
  const int32_t* wg = sc.in_map<const int32_t>(sc.o_wg);
  for (int d = 0; d < 5; ++d)
    for (int k = 0; k < 3; ++k) {
      const std::vector<int32_t>& v = sc.list[d][k];
      if (v.empty()) continue;
      size_t lds = 0;
      for (int32_t p : v) lds = std::max(lds, sc.need[(size_t)p]);
      HIPCHK(c, launch(wg, (int)v.size(), d, lds));
      wg += v.size();
    }
  if (sc.prof) HIPCHK(c, hipEventRecord(sc.ev[1], sc.st));
  return AGP_OK;
}

// the end of the profiled read-out span: behind the entry's read-out kernels, ahead of the copies
int series_mark_readout(agp_ctx* c, SeriesCall& sc) {
  if (sc.prof) HIPCHK(c, hipEventRecord(sc.ev[2], sc.st));
  sc.readout = sc.prof;
  return AGP_OK;
}

// The call's read-back: the pinned landing zone at the size of [logpdf | info] and everything the entry registered, one copy each
// in that order (an array of 0 bytes: none), and the stream drained.
int series_fetch(agp_ctx* c, SeriesCall& sc) {
  size_t total = sc.values_bytes();
  for (SeriesCall::Back& b : sc.back) { b.off = (total + 7) & ~(size_t)7; total = b.off + b.bytes; }
  HIPCHK(c, sc.s->h_out.ensure(total));
  char* ho = static_cast<char*>(sc.s->h_out.p);
  HIPCHK(c, hipMemcpyAsync(ho, sc.s->out_lp.p, sc.values_bytes(), hipMemcpyDeviceToHost, sc.st));
  for (const SeriesCall::Back& b : sc.back)
    if (b.bytes > 0) HIPCHK(c, hipMemcpyAsync(ho + b.off, b.dev, b.bytes, hipMemcpyDeviceToHost, sc.st));
  HIPCHK(c, hipStreamSynchronize(sc.st));
  return AGP_OK;
}

// ... and out of its head into the caller's arrays.  An empty series (never launched, or launched for the prior predictive):
// the value is 0 either way
void series_copy_values(const SeriesCall& sc, double* out_logpdf, int32_t* out_info) {
  const int P = sc.pp.P;
  const double* hl = static_cast<const double*>(sc.s->h_out.p);
  const int32_t* hi = reinterpret_cast<const int32_t*>(hl + P);
  for (int p = 0; p < P; ++p) {
    const bool empty = sc.len[(size_t)p] == 0;
    if (out_logpdf) out_logpdf[p] = empty ? 0.0 : hl[p];
    out_info[p] = empty ? 0 : hi[p];
  }
}

// agp_get_timing: out[0] = out[2] = the value kernels of the call (covariance, factorisation, solve and value are one kernel);
// out[4] = the band's three read-out kernels, the held-out entry's mixture read-out, the sampling entry's NaN fill (0 in the others)
int series_timing(agp_ctx* c, const SeriesCall& sc) {
  if (!sc.prof) return AGP_OK;
  float ms = 0.f, readout_ms = 0.f;
  if (sc.readout) HIPCHK(c, hipEventElapsedTime(&readout_ms, sc.ev[1], sc.ev[2]));
  HIPCHK(c, hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]));
  std::lock_guard<std::mutex> g(c->mu);
  for (double& t : c->timing) t = 0.0;
  c->timing[0] = ms; c->timing[2] = ms;
  c->timing[4] = readout_ms;
  return AGP_OK;
}

// The long kernel's launches of one class: the particles hv[0 .. grid) (longest first) in chunks whose workspaces fit `limit` bytes
// together — every workgroup of a chunk gets the chunk's largest workspace, that of its first particle (sc.ws_blocks: the mode's
// blocks per workgroup); a chunk is never empty.  f(first, count, stride in doubles) -> hipError_t.
template <class F> hipError_t long_chunks(const SeriesCall& sc, const int32_t* hv, int grid, int64_t limit, F&& f) {
  for (int i = 0; i < grid;) {
    const int nb = (sc.len[(size_t)hv[i]] + BS - 1) / BS;
    const long long stride = sc.ws_blocks(nb) * 256;
    const int cnt = (int)std::max<int64_t>(1, std::min<int64_t>(grid - i, limit / (int64_t)(stride * sizeof(double))));
    if (const hipError_t e = f(i, cnt, stride)) return e;
    i += cnt;
  }
  return hipSuccess;
}

// the long launches' workspace (the slot's A) at the size of the call's largest chunk, before anything is launched: the launches
// share it in stream order.  Bounded by the call's workspace limit and 1 GiB.  A call without long classes takes none.
int series_long_workspace(agp_ctx* c, SeriesCall& sc) {
  sc.ws_limit = std::min<int64_t>(ws_limit_bytes(c), (int64_t)1 << 30);
  size_t ws_bytes = 0;
  const int32_t* hv = sc.wg.data();
  for (int d = 0; d < 5; ++d)
    for (int k = 0; k < 3; ++k) {
      const int grid = (int)sc.list[d][k].size();
      if (d >= SERIES_LONG_CLASS)
        (void)long_chunks(sc, hv, grid, sc.ws_limit, [&](int, int cnt, long long stride) {
          ws_bytes = std::max(ws_bytes, sizeof(double) * (size_t)cnt * (size_t)stride);
          return hipSuccess;
        });
      hv += grid;
    }
  if (ws_bytes > 0) HIPCHK(c, sc.s->A.ensure(ws_bytes));
  return AGP_OK;
}

// one long class of a staged call (series_launch's wg, grid), chunk by chunk: la is the kernel's arguments but for wg and the
// workspace; launch(la, count) -> hipError_t
template <class Args, class Launch>
hipError_t series_launch_long(agp_ctx* c, SeriesCall& sc, const int32_t* wg, int grid, Args la, Launch&& launch) {
  const int32_t* hv = sc.wg.data() + (wg - sc.in_map<const int32_t>(sc.o_wg));
  return long_chunks(sc, hv, grid, sc.ws_limit, [&](int first, int cnt, long long stride) {
    // (NaN-poison mode: a later launch must not find an earlier one's finished blocks in the workspace)
    if (sc.ws_used && c->poison.active())
      if (const hipError_t e = sc.s->A.poison_async(sc.st)) return e;
    sc.ws_used = true;
    la.wg = wg + first;
    la.ws = sc.s->A.as<double>(); la.ws_stride = stride;
    return launch(la, cnt);
  });
}

// the predictive launches of a staged call with queries: means and variances into pred_mean / pred_var, where they stay.  The long
// classes of mode long_prediction (series_long_workspace has run): k_long_series_predict, chunk by chunk.
int series_launch_predict(agp_ctx* c, SeriesCall& sc) {
  Slot* s = sc.s;
  SeriesPredArgs pa = {};
  series_query_args(sc, pa);
  pa.out_mean = s->pred_mean.as<double>(); pa.out_var = s->pred_var.as<double>();
  return series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    if (d < SERIES_LONG_CLASS) {
      pa.wg = wg;
      return launch_series_predict(sc.st, pa, grid, d == 0 ? 4 : 8, lds);
    }
    LongSeriesPredArgs la = {};
    static_cast<SeriesPredArgs&>(la) = pa;
    return series_launch_long(c, sc, wg, grid, la, [&](const LongSeriesPredArgs& a, int cnt) {
      return launch_long_series_predict(sc.st, a, cnt, d == SERIES_LONG_CLASS ? 4 : 8, lds);
    });
  });
}

// mode value: agp_logpdf_series_batch; mode long_value: agp_logpdf_long_series_batch — the same stages, the long particles' launches
// (classes SERIES_LONG_CLASS ..) with a workspace out of the slot's A, split where the call's workspace limit asks for it
int logpdf_series(agp_ctx* c, SeriesCall& sc, double* out_logpdf, int32_t* out_info, SeriesMode mode = SeriesMode::value) {
  STAGE(series_check_sizes(c, sc));
  if (sc.pp.P == 0) return AGP_OK;
  STAGE(series_check_pointers(c, sc, out_logpdf && out_info));
  STAGE(series_check_layout(c, sc));
  STAGE(series_classes(c, sc, mode));
  if (sc.wg.empty()) { series_zero_values(sc, out_logpdf, out_info); return AGP_OK; }
  STAGE(series_stage(c, sc));
  STAGE(series_long_workspace(c, sc));
  HIPCHK(c, sc.up.flush(sc.s->h_stage, sc.s->up_blob, sc.st));
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    if (d < SERIES_LONG_CLASS) {
      SeriesArgs a = sc.sa;
      a.wg = wg;
      return launch_series_logpdf(sc.st, a, grid, d == 0 ? 4 : 8, lds);
    }
    LongSeriesArgs la = {};
    static_cast<SeriesArgs&>(la) = sc.sa;
    return series_launch_long(c, sc, wg, grid, la, [&](const LongSeriesArgs& a, int cnt) {
      return launch_long_series_logpdf(sc.st, a, cnt, d == SERIES_LONG_CLASS ? 4 : 8, lds);
    });
  }));
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  return series_timing(c, sc);
}

// also out_grad (agp_logpdf_grad_batch's layout) and out_gnoise
int logpdf_grad_series(agp_ctx* c, SeriesCall& sc, double* out_logpdf, double* out_grad, double* out_gnoise, int32_t* out_info) {
  const int P = sc.pp.P;
  STAGE(series_check_sizes(c, sc));
  if (P == 0) return AGP_OK;
  STAGE(series_check_pointers(c, sc, out_logpdf && out_info));
  const size_t n_prm_total = (size_t)std::max(0, sc.pp.prm_off[P]);
  if (!out_gnoise) return fail(c, AGP_ERR_ARG, "null pointer argument (out_grad_noise)");
  if (!out_grad && sc.pp.prm_off[P] > 0) return fail(c, AGP_ERR_ARG, "null pointer argument (out_grad with parameters present)");
  STAGE(series_check_layout(c, sc));
  STAGE(series_classes(c, sc, SeriesMode::gradient));
  if (sc.wg.empty()) {
    series_zero_values(sc, out_logpdf, out_info);
    std::fill(out_gnoise, out_gnoise + P, 0.0); std::fill(out_grad, out_grad + n_prm_total, 0.0);
    return AGP_OK;
  }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  SeriesGradArgs ga = {};
  STAGE(series_grad_tape(c, sc, ga));
  HIPCHK(c, s->dgrad.ensure(sizeof(double) * std::max<size_t>(1, n_prm_total)));
  HIPCHK(c, s->dgnoise.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  ga.out_grad = s->dgrad.as<double>(); ga.out_gnoise = s->dgnoise.as<double>();
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    ga.wg = wg;
    return launch_series_logpdf_grad(sc.st, ga, grid, d == 2 ? 8 : 4, d == 0 ? 16 : 64, lds);
  }));
  const int b_gn = sc.want(s->dgnoise.p, sizeof(double) * (size_t)P), b_gr = sc.want(s->dgrad.p, sizeof(double) * n_prm_total);
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  // (an empty series: zeros; a bad pivot: NaN in the whole block — the kernel wrote them, slot by slot through gmap)
  const double* hgn = sc.got<double>(b_gn);
  const double* hgr = sc.got<double>(b_gr);
  for (int p = 0; p < P; ++p) {
    const bool empty = sc.len[(size_t)p] == 0;
    out_gnoise[p] = empty ? 0.0 : hgn[p];
    for (int32_t q = sc.pp.prm_off[p]; q < sc.pp.prm_off[p + 1]; ++q) out_grad[q] = empty ? 0.0 : hgr[q];
  }
  return series_timing(c, sc);
}

// The chain of agp_hmc_series_batch: the latent state, the transform classes, the schedule and the outputs (host).
struct SeriesHmcCall {
  const double* z; const double* z_noise; const int32_t* prm_class; int32_t C; const double* tf; int32_t noise_class; double noise_jitter;
  int32_t n_hmc, L_prm; double eps_prm; int32_t L_noise; double eps_noise; int32_t n_exit; const uint64_t* seeds; int32_t flags;
  double* out_z; double* out_z_noise; double* out_prm; double* out_noise; int32_t* out_counts; double* out_trace;
};

// theta = transform(z) on the host (the programs are compiled from the initial state; the device forms every value it uses itself)
double hmc_transform_host(const double* tf, int c, double z) {
  const double x = tf[3 * c] + tf[3 * c + 1] * z, sc = tf[3 * c + 2];
  return sc == 0.0 ? std::exp(x) : sc / (1.0 + std::exp(-x));
}

// rejuvenate_particle_parameters for every (series, particle) in one call: k_series_hmc, the gradient kernel's statements in a loop.
// sc.pp carries the programs; its prm / noise are filled here from the initial state.
int hmc_series(agp_ctx* c, SeriesCall& sc, const SeriesHmcCall& hm, double* out_logpdf, int32_t* out_info) {
  const int P = sc.pp.P;
  char buf[256];
  STAGE(series_check_sizes(c, sc));
  if (P == 0) return AGP_OK;
  if (!(sc.pt_off && sc.ts && sc.xs && sc.series && sc.pp.op_off && sc.pp.ops && sc.pp.prm_off)) return fail(c, AGP_ERR_ARG, "null pointer argument");
  if (!(out_logpdf && out_info && hm.out_z_noise && hm.out_noise && hm.out_counts)) return fail(c, AGP_ERR_ARG, "null pointer argument (outputs)");
  if (!(hm.z_noise && hm.tf && hm.seeds)) return fail(c, AGP_ERR_ARG, "null pointer argument (z_noise, tf or seeds)");
  const size_t NT = (size_t)std::max(0, sc.pp.prm_off[P]);
  if (NT > 0 && !(hm.z && hm.prm_class)) return fail(c, AGP_ERR_ARG, "null pointer argument (z or prm_class with parameters present)");
  if (NT > 0 && !(hm.out_z && hm.out_prm)) return fail(c, AGP_ERR_ARG, "null pointer argument (out_z or out_prm with parameters present)");
  if (hm.n_hmc < 0 || hm.L_prm < 0 || hm.L_noise < 0 || !(hm.eps_prm >= 0.0) || !(hm.eps_noise >= 0.0))
    return fail(c, AGP_ERR_ARG, "n_hmc, L_param, L_noise, eps_param and eps_noise must not be negative");
  if (hm.n_hmc > (1 << 20) || hm.L_prm > (1 << 20) || hm.L_noise > (1 << 20)) return fail(c, AGP_ERR_ARG, "n_hmc, L_param and L_noise are limited to 2^20");
  if (hm.C < 1 || hm.C > 4096) return fail(c, AGP_ERR_ARG, "the transform table needs between 1 and 4096 classes");
  for (int k = 0; k < hm.C; ++k)
    if (!(hm.tf[3 * k + 1] > 0.0) || !(hm.tf[3 * k + 2] >= 0.0) || !std::isfinite(hm.tf[3 * k]) || !std::isfinite(hm.tf[3 * k + 1]) || !std::isfinite(hm.tf[3 * k + 2])) {
      snprintf(buf, sizeof buf, "transform class %d: (mu, sigma, scale) must be finite with sigma > 0 and scale >= 0", k);
      return fail(c, AGP_ERR_ARG, buf);
    }
  if (hm.noise_class < 0 || hm.noise_class >= hm.C) {
    snprintf(buf, sizeof buf, "noise class %d outside [0, %d)", (int)hm.noise_class, (int)hm.C);
    return fail(c, AGP_ERR_ARG, buf);
  }
  STAGE(series_check_layout(c, sc));
  for (int p = 0; p < P; ++p)
    for (int32_t q = sc.pp.prm_off[p]; q < sc.pp.prm_off[p + 1]; ++q)
      if (hm.prm_class[q] >= hm.C) {
        snprintf(buf, sizeof buf, "particle %d: parameter %d has transform class %d, outside the table's %d", p, (int)(q - sc.pp.prm_off[p]),
                 (int)hm.prm_class[q], (int)hm.C);
        return fail(c, AGP_ERR_ARG, buf);
      }
  // the initial state in parameter space: what the programs are compiled from, and what a particle that is never launched returns
  std::vector<double> th0(std::max<size_t>(1, NT)), nz0((size_t)P);
  for (size_t q = 0; q < NT; ++q) th0[q] = hm.prm_class[q] < 0 ? hm.z[q] : hmc_transform_host(hm.tf, hm.prm_class[q], hm.z[q]);
  for (int p = 0; p < P; ++p) nz0[(size_t)p] = hmc_transform_host(hm.tf, hm.noise_class, hm.z_noise[p]) + hm.noise_jitter;
  sc.pp.prm = th0.data(); sc.pp.noise = nz0.data();
  sc.hmc_C = hm.C;
  STAGE(series_classes(c, sc, SeriesMode::hmc));
  const Batch& bt = sc.bt;
  // the slot map: the value and the gradient program number their parameter slots alike (emit / emit_grad walk the tree in one
  // order), gmap names the caller parameter of a slot and the node's kind the derivation rule — checked against the compiled values
  std::vector<uint8_t> rule(bt.gprm.size(), (uint8_t)HMC_RULE_COPY);
  for (int p = 0; p < P; ++p) {
    const ProgHdr& h = bt.hdr[(size_t)p];
    const GProgHdr& g = bt.ghdr[(size_t)p];
    bool ok = h.n_prm == g.n_prm && g.n_prm == sc.pp.prm_off[p + 1] - sc.pp.prm_off[p];
    for (int i = 0; ok && i < g.n_ops; ++i) {
      const int o = bt.gops[(size_t)g.node_off + i];
      const size_t po = (size_t)g.prm_off + bt.gpoff[(size_t)g.node_off + i];
      if (o == OP_SE) rule[po] = HMC_RULE_INV_SQ;
      else if (o == OP_GE) rule[po] = HMC_RULE_INV;
      else if (o == OP_PER) { rule[po] = HMC_RULE_M2_INV_SQ; rule[po + 1] = HMC_RULE_PI_OVER; }
    }
    for (int q = 0; ok && q < g.n_prm; ++q) {
      const double want = bt.prm[(size_t)h.prm_off + q], got = hmc_rule_apply(rule[(size_t)g.prm_off + q], bt.gprm[(size_t)g.prm_off + q]);
      ok = std::memcmp(&want, &got, sizeof want) == 0 || (want != want && got != got);
    }
    if (!ok) return fail(c, AGP_ERR_HOST, "internal error: the value and the gradient program disagree on their parameter slots");
  }
  // what a particle on an empty series returns (never launched): the transformed inputs, value 0, no move
  const size_t tr_n = hm.out_trace ? (size_t)4 * hm.n_hmc : 0;
  auto unmoved = [&](int p) {
    for (int32_t q = sc.pp.prm_off[p]; q < sc.pp.prm_off[p + 1]; ++q) { hm.out_z[q] = hm.z[q]; hm.out_prm[q] = th0[(size_t)q]; }
    hm.out_z_noise[p] = hm.z_noise[p]; hm.out_noise[p] = nz0[(size_t)p];
    std::fill(hm.out_counts + 4 * (size_t)p, hm.out_counts + 4 * (size_t)p + 4, 0);
    if (tr_n) std::fill(hm.out_trace + tr_n * p, hm.out_trace + tr_n * (p + 1), std::numeric_limits<double>::quiet_NaN());
    out_logpdf[p] = 0.0; out_info[p] = 0;
  };
  if (sc.wg.empty()) {
    for (int p = 0; p < P; ++p) unmoved(p);
    return AGP_OK;
  }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  SeriesHmcArgs ha = {};      // (out_grad, out_gnoise: null — the chain keeps its gradients to itself)
  STAGE(series_grad_tape(c, sc, ha));
  // hmc_in  = [z (NT) | z_noise (P) | tf (3 C) | seeds (P) | params | prm_class (NT ints) | rule (bytes)]
  // hmc_out = [out_z (NT) | out_prm (NT) | out_z_noise (P) | out_noise (P) | trace (P tr_n) | counts (4 P ints)]
  const size_t D = sizeof(double);
  const size_t i_zn = D * NT, i_tf = i_zn + D * P, i_seed = i_tf + D * 3 * hm.C, i_par = i_seed + D * P;
  const size_t i_cls = i_par + ((sizeof(SeriesHmcParams) + 7) & ~(size_t)7), i_rule = i_cls + sizeof(int32_t) * NT;
  const size_t o_prm = D * NT, o_zn = 2 * D * NT, o_nz = o_zn + D * P, o_tr = o_nz + D * P, o_cnt = o_tr + D * tr_n * P;
  const size_t out_bytes = o_cnt + sizeof(int32_t) * 4 * P;
  HIPCHK(c, s->hmc_in.ensure(i_rule + rule.size() + 8));
  HIPCHK(c, s->hmc_out.ensure(out_bytes));
  char* di = s->hmc_in.as<char>();
  char* dout = s->hmc_out.as<char>();
  SeriesHmcParams par = {};
  par.z = reinterpret_cast<const double*>(di); par.z_noise = reinterpret_cast<const double*>(di + i_zn);
  par.tf = reinterpret_cast<const double*>(di + i_tf); par.seeds = reinterpret_cast<const unsigned long long*>(di + i_seed);
  par.cls = reinterpret_cast<const int32_t*>(di + i_cls); par.rule = reinterpret_cast<const uint8_t*>(di + i_rule);
  par.C = hm.C; par.noise_class = hm.noise_class; par.noise_jitter = hm.noise_jitter;
  par.n_hmc = hm.n_hmc; par.L_prm = hm.L_prm; par.L_noise = hm.L_noise; par.n_exit = hm.n_exit; par.flags = hm.flags;
  par.eps_prm = hm.eps_prm; par.eps_noise = hm.eps_noise;
  par.out_z = reinterpret_cast<double*>(dout); par.out_prm = reinterpret_cast<double*>(dout + o_prm);
  par.out_z_noise = reinterpret_cast<double*>(dout + o_zn); par.out_noise = reinterpret_cast<double*>(dout + o_nz);
  par.out_trace = tr_n ? reinterpret_cast<double*>(dout + o_tr) : nullptr;
  par.out_counts = reinterpret_cast<int32_t*>(dout + o_cnt);
  sc.up.add(di, hm.z, D * NT);
  sc.up.add(di + i_zn, hm.z_noise, D * P);
  sc.up.add(di + i_tf, hm.tf, D * 3 * hm.C);
  sc.up.add(di + i_seed, hm.seeds, D * P);
  sc.up.add(di + i_par, &par, sizeof par);
  sc.up.add(di + i_cls, hm.prm_class, sizeof(int32_t) * NT);
  sc.up.add(di + i_rule, rule.data(), rule.size());
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  ha.hm = reinterpret_cast<const SeriesHmcParams*>(di + i_par); ha.C = hm.C;
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    ha.wg = wg;
    return launch_series_hmc(sc.st, ha, grid, d == 2 ? 8 : 4, d == 0 ? 16 : 64, lds);
  }));
  const int b_out = sc.want(dout, out_bytes);
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  const char* hb = sc.got<char>(b_out);
  const double* hz = reinterpret_cast<const double*>(hb);
  const double* hp = reinterpret_cast<const double*>(hb + o_prm);
  const double* hzn = reinterpret_cast<const double*>(hb + o_zn);
  const double* hnz = reinterpret_cast<const double*>(hb + o_nz);
  const double* htr = reinterpret_cast<const double*>(hb + o_tr);
  const int32_t* hcn = reinterpret_cast<const int32_t*>(hb + o_cnt);
  for (int p = 0; p < P; ++p) {
    if (sc.len[(size_t)p] == 0) { unmoved(p); continue; }
    for (int32_t q = sc.pp.prm_off[p]; q < sc.pp.prm_off[p + 1]; ++q) { hm.out_z[q] = hz[q]; hm.out_prm[q] = hp[q]; }
    hm.out_z_noise[p] = hzn[p]; hm.out_noise[p] = hnz[p];
    std::copy(hcn + 4 * (size_t)p, hcn + 4 * (size_t)p + 4, hm.out_counts + 4 * (size_t)p);
    if (tr_n) std::copy(htr + tr_n * p, htr + tr_n * (p + 1), hm.out_trace + tr_n * p);
  }
  return series_timing(c, sc);
}

// also the posterior at the series' query times, particle-major behind out_off; out_logpdf may be null.  mode prediction:
// agp_predict_series_batch; mode long_prediction: agp_predict_long_series_batch — the same stages, the long particles' launches with
// their workspace (series_long_workspace, series_launch_predict)
int predict_series(agp_ctx* c, SeriesCall& sc, double* out_mean, double* out_var, int64_t* out_off, double* out_logpdf,
                   int32_t* out_info, SeriesMode mode = SeriesMode::prediction) {
  STAGE(series_check_sizes(c, sc));
  if (sc.pp.P == 0) return AGP_OK;
  STAGE(series_check_pointers(c, sc, out_info != nullptr));
  if (!sc.q_off || !sc.ts_pred || !out_mean || !out_var || !out_off)
    return fail(c, AGP_ERR_ARG, "null pointer argument (q_off, ts_pred, out_mean, out_var or out_off)");
  STAGE(series_check_layout(c, sc));
  STAGE(series_classes(c, sc, mode));
  std::copy(sc.ooff.begin(), sc.ooff.end(), out_off);      // (no check is left to fail, nothing is launched yet)
  if (sc.wg.empty()) { series_zero_values(sc, out_logpdf, out_info); return AGP_OK; }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  STAGE(series_long_workspace(c, sc));
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  STAGE(series_launch_predict(c, sc));
  const size_t n_out = sc.n_out();
  const int b_mean = sc.want(s->pred_mean.p, sizeof(double) * n_out), b_var = sc.want(s->pred_var.p, sizeof(double) * n_out);
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  // every particle with query points was launched and wrote its whole block
  std::copy_n(sc.got<double>(b_mean), n_out, out_mean);
  std::copy_n(sc.got<double>(b_var), n_out, out_var);
  return series_timing(c, sc);
}

// The band of every series' mixture: predict_series' launches, their means and variances left on the device for the read-out
// kernels behind them on the same stream.  out_logpdf may be null.  mode long_prediction: agp_predict_quantile_long_series_batch.
int predict_quantile_series(agp_ctx* c, SeriesCall& sc, const SeriesQuantOut& qo, double* out_logpdf, int32_t* out_info,
                            SeriesMode mode = SeriesMode::prediction) {
  const int P = sc.pp.P;
  const int32_t S = sc.S;
  STAGE(series_check_sizes(c, sc));
  STAGE(series_check_pointers(c, sc, out_info != nullptr));
  if (!sc.q_off || !sc.ts_pred) return fail(c, AGP_ERR_ARG, "null pointer argument (q_off, ts_pred, out_mean, out_var or out_off)");
  STAGE(series_check_layout(c, sc));
  MixPlan qp;
  STAGE(quant_plan(c, S, P, sc.series, sc.q_off, qo, qp));
  if (P == 0) { quant_fill_nan(qo, 0, qp.Q, qo.nq); return AGP_OK; }      // (S series without a particle)
  STAGE(series_classes(c, sc, mode));
  if (sc.wg.empty()) {
    series_zero_values(sc, out_logpdf, out_info);
    quant_fill_nan(qo, 0, qp.Q, qo.nq);      // (only series without a particle have query points here)
    return AGP_OK;
  }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  STAGE(series_long_workspace(c, sc));
  // x and the moments in sq_out, the flags in sq_flag = [converged | iterations | first_bad (P) | bad (S)]
  const size_t nx = qp.Q * (size_t)qo.nq;
  const bool want_mom = qo.mix_mean || qo.mix_var;
  MixTabs mt;
  STAGE(series_stage_mix(c, sc, qp, mt));
  HIPCHK(c, s->sq_w.ensure(sizeof(double) * std::max<size_t>(1, qp.vals.size())));
  HIPCHK(c, s->sq_cm.ensure(sizeof(double) * std::max<size_t>(1, qp.R)));
  HIPCHK(c, s->sq_cs.ensure(sizeof(double) * std::max<size_t>(1, qp.R)));
  HIPCHK(c, s->sq_out.ensure(sizeof(double) * std::max<size_t>(1, nx + 2 * qp.Q)));
  HIPCHK(c, s->sq_flag.ensure(sizeof(int32_t) * (2 * nx + (size_t)P + (size_t)S)));
  sc.up.add(s->sq_w.p, qp.vals.data(), sizeof(double) * qp.vals.size());
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  STAGE(series_launch_predict(c, sc));
  SeriesQuantArgs qa = {};
  qa.S = S; qa.nq = (int)qo.nq;
  qa.pt_off = sc.sa.pt_off;
  qa.q_off = sc.in_map<const long long>(sc.o_qoff);
  qa.out_off = sc.in_map<const long long>(sc.o_ooff);
  qa.mean = s->pred_mean.as<double>(); qa.var = s->pred_var.as<double>(); qa.pred_info = sc.sa.out_info;
  qa.pl_off = mt.pl_off; qa.w_off = mt.w_off; qa.row_off = mt.row_off; qa.plist = mt.plist;
  qa.w = s->sq_w.as<double>(); qa.slope = qa.w + qp.W; qa.intercept = qa.slope + S; qa.ivar = qa.intercept + S; qa.q = qa.ivar + S;
  qa.tol = qo.tol; qa.max_iter = (long long)qo.max_iter;
  qa.cm = s->sq_cm.as<double>(); qa.cs = s->sq_cs.as<double>();
  qa.out_x = s->sq_out.as<double>();
  qa.out_mean = want_mom ? qa.out_x + nx : nullptr; qa.out_var = want_mom ? qa.out_x + nx + qp.Q : nullptr;
  qa.out_conv = s->sq_flag.as<int32_t>(); qa.out_iters = qa.out_conv + nx;
  qa.first_bad = qa.out_iters + nx; qa.bad = qa.first_bad + P;
  launch_series_mix_readout(sc.st, qa, (long long)qp.Q, qp.max_rows_el);
  HIPCHK(c, hipGetLastError());
  STAGE(series_mark_readout(c, sc));
  // back: [x (nx) | mean (Q) | var (Q)], the moments when wanted, and [converged (nx) | iterations (nx) | first_bad (P)]
  const int b_band = sc.want(s->sq_out.p, sizeof(double) * (nx + (want_mom ? 2 * qp.Q : 0)));
  const int b_flag = sc.want(s->sq_flag.p, sizeof(int32_t) * (2 * nx + (size_t)P));
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  const double* hb = sc.got<double>(b_band);
  const int32_t* hf = sc.got<int32_t>(b_flag);
  // raw_components' rule: a particle whose predictive exists but whose raw mean or variance is unusable at query i reports n_s + i + 1
  for (int p = 0; p < P; ++p)
    if (out_info[p] == 0 && sc.nq[(size_t)p] > 0 && hf[2 * nx + (size_t)p] != 0) out_info[p] = hf[2 * nx + (size_t)p];
  if (qo.x) std::copy(hb, hb + nx, qo.x);
  if (qo.conv) std::copy(hf, hf + nx, qo.conv);
  if (qo.iters) std::copy(hf + nx, hf + 2 * nx, qo.iters);
  if (qo.mix_mean) std::copy(hb + nx, hb + nx + qp.Q, qo.mix_mean);
  if (qo.mix_var) std::copy(hb + nx + qp.Q, hb + nx + 2 * qp.Q, qo.mix_var);
  return series_timing(c, sc);
}

// The held-out side of agp_predict_logpdf_series_batch: values, transforms, mixture weights, and the outputs beside [logpdf | info].
struct SeriesProbaOut {
  const double* y_pred;      // [q_off[S]] held-out values, in the space of xs
  const double* y_slope;     // [S] or null (1)
  const double* weights;     // [P] or null: no mixtures
  double* terms;             // [out_off[P]] or null
  int64_t* out_off;          // [P + 1] or null
  double* series_logp;       // [S]; null exactly when weights is
};

// The log-density of every series' held-out values under each of its particles: the value kernel on the joint points, the
// mixtures' read-out behind it on the same stream.  mode held_out: agp_predict_logpdf_series_batch; mode long_held_out:
// agp_predict_logpdf_long_series_batch — the same stages, the joint size checked against the entry's cap (sc.max_n), the long particles'
// launches (classes SERIES_LONG_CLASS ..) with the value kernel's workspace out of the slot's A, split where the call's workspace
// limit asks for it
int predict_logpdf_series(agp_ctx* c, SeriesCall& sc, const SeriesProbaOut& po, double* out_logpdf, int32_t* out_info,
                          SeriesMode mode = SeriesMode::held_out) {
  const int P = sc.pp.P;
  const int32_t S = sc.S;
  char buf[256];
  STAGE(series_check_sizes(c, sc));
  if ((po.weights == nullptr) != (po.series_logp == nullptr))
    return fail(c, AGP_ERR_ARG, "weights and out_series_logp must both be given or both be NULL");
  if (P == 0 && !po.weights) return AGP_OK;
  STAGE(series_check_pointers(c, sc, out_logpdf && out_info));
  if (!sc.q_off || !sc.ts_pred) return fail(c, AGP_ERR_ARG, "null pointer argument (q_off or ts_pred)");
  STAGE(series_check_layout(c, sc));
  const size_t Q = S > 0 ? (size_t)sc.q_off[S] : 0;
  if (!po.y_pred && Q > 0) return fail(c, AGP_ERR_ARG, "null pointer argument (y_pred with held-out points present)");
  std::vector<double> slope((size_t)S);
  for (int32_t s = 0; s < S; ++s) {
    STAGE(series_check_joint(c, sc, s, "held-out", sc.max_n, sc.max_name));
    for (long long j = 0, m = sc.q_off[s + 1] - sc.q_off[s]; j < m; ++j)
      if (!std::isfinite(po.y_pred[sc.q_off[s] + j])) {
        snprintf(buf, sizeof buf, "series %d: held-out value %lld is not finite", (int)s, j);
        return fail(c, AGP_ERR_ARG, buf);
      }
    double icpt;
    STAGE(series_y_transform(c, s, po.y_slope, nullptr, slope[(size_t)s], icpt));
  }
  MixPlan qp;      // the mixtures' lists and weights (the transforms: checked above)
  if (po.weights) STAGE(mix_plan(c, S, P, sc.series, sc.q_off, po.weights, nullptr, nullptr, 0, qp));
  const double nanv = std::numeric_limits<double>::quiet_NaN();
  if (P == 0) { std::fill(po.series_logp, po.series_logp + S, nanv); return AGP_OK; }      // (S series without a particle)
  STAGE(series_classes(c, sc, mode));
  if (po.out_off) std::copy(sc.ooff.begin(), sc.ooff.end(), po.out_off);      // (no check is left to fail, nothing is launched yet)
  if (sc.wg.empty()) {      // nothing held out for any particle: every score is 0, and so is every mixture's
    series_zero_values(sc, out_logpdf, out_info);
    for (int32_t s = 0; s < S && po.series_logp; ++s) po.series_logp[s] = qp.tab[(size_t)s + 1] > qp.tab[(size_t)s] ? 0.0 : nanv;
    return AGP_OK;
  }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  STAGE(series_long_workspace(c, sc));
  // sq_w = [y_pred (Q) | slope (S) | the plan's values: w (W) ..]; sq_tab = [pl_off | w_off | row_off | plist]; sq_out = the mixtures (S)
  MixTabs mt = {};
  HIPCHK(c, s->sq_w.ensure(sizeof(double) * std::max<size_t>(1, Q + (size_t)S + qp.vals.size())));
  sc.up.add(s->sq_w.p, po.y_pred, sizeof(double) * Q);
  sc.up.add(s->sq_w.as<double>() + Q, slope.data(), sizeof(double) * (size_t)S);
  if (po.weights) {
    STAGE(series_stage_mix(c, sc, qp, mt));
    HIPCHK(c, s->sq_out.ensure(sizeof(double) * (size_t)S));
    sc.up.add(s->sq_w.as<double>() + Q + S, qp.vals.data(), sizeof(double) * qp.vals.size());
  }
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  SeriesProbaArgs pa = {};
  series_query_args(sc, pa);
  pa.y_pred = s->sq_w.as<double>(); pa.y_slope = s->sq_w.as<double>() + Q;
  pa.out_terms = po.terms ? s->pred_mean.as<double>() : nullptr;
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    if (d < SERIES_LONG_CLASS) {
      pa.wg = wg;
      return launch_series_predict_logpdf(sc.st, pa, grid, d == 0 ? 4 : 8, lds);
    }
    LongSeriesProbaArgs la = {};
    static_cast<SeriesProbaArgs&>(la) = pa;
    return series_launch_long(c, sc, wg, grid, la, [&](const LongSeriesProbaArgs& a, int cnt) {
      return launch_long_series_predict_logpdf(sc.st, a, cnt, d == SERIES_LONG_CLASS ? 4 : 8, lds);
    });
  }));
  if (po.weights) {
    SeriesMixLogpArgs ma = {};
    ma.S = S;
    ma.q_off = pa.q_off;
    ma.pl_off = mt.pl_off; ma.w_off = mt.w_off; ma.plist = mt.plist;
    ma.w = s->sq_w.as<double>() + Q + S;
    ma.lp = sc.sa.out_lp; ma.info = sc.sa.out_info;
    ma.out = s->sq_out.as<double>();
    launch_series_mix_logp(sc.st, ma);
    HIPCHK(c, hipGetLastError());
    STAGE(series_mark_readout(c, sc));
  }
  // back: the terms and the mixtures, each when wanted
  const size_t n_terms = po.terms ? sc.n_out() : 0;
  const int b_terms = sc.want(s->pred_mean.p, sizeof(double) * n_terms);
  const int b_mix = sc.want(s->sq_out.p, sizeof(double) * (po.weights ? (size_t)S : 0));
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);      // (nothing held out: length 0 here, so 0 and info 0)
  // every particle with held-out points was launched and wrote its whole block
  if (n_terms > 0) std::copy_n(sc.got<double>(b_terms), n_terms, po.terms);
  if (po.weights) std::copy_n(sc.got<double>(b_mix), S, po.series_logp);
  return series_timing(c, sc);
}

// The sampling side of agp_predict_sample_series_batch: transforms, mixture weights, the draws, and the outputs beside info.
struct SeriesSampleOut {
  const double* y_slope;       // [S] or null (1)
  const double* y_intercept;   // [S] or null (0)
  const double* weights;       // [P] particle p's weight inside its series' mixture
  int64_t R;                   // samples per series
  const uint64_t* seeds;       // [S]; may be null when both component and z are given (or R == 0)
  const int32_t* component;    // [S R] global particle indices, or null: drawn
  const double* z;             // [R q_off[S]] or null: drawn
  double* x;                   // [R q_off[S]]
  int32_t* out_component;      // [S R] or null
  double* mean; int64_t* out_off;      // [out_off[P]], [P + 1]; mean nullable
  double* cov; int64_t* cov_off;       // [cov_off[P]], [P + 1]; cov nullable
};

// Samples of every series' mixture and the mixtures' components: the held-out entry's factorisation with a zero query right-hand
// side, the query rows read out in the same launches, the NaN fill of failed series behind them on the same stream.
int predict_sample_series(agp_ctx* c, SeriesCall& sc, const SeriesSampleOut& so, int32_t* out_info) {
  const int P = sc.pp.P;
  const int32_t S = sc.S;
  const int64_t R = so.R;
  char buf[256];
  STAGE(series_check_sizes(c, sc));
  if (R < 0) return fail(c, AGP_ERR_ARG, "negative number of samples (R)");
  if (P == 0 && (S == 0 || R == 0)) return AGP_OK;
  if (P == 0) return fail(c, AGP_ERR_ARG, "series 0 has no particles to sample from");
  STAGE(series_check_pointers(c, sc, out_info != nullptr));
  if (!sc.q_off || !sc.ts_pred) return fail(c, AGP_ERR_ARG, "null pointer argument (q_off or ts_pred)");
  if ((so.mean && !so.out_off) || (so.cov && !so.cov_off))
    return fail(c, AGP_ERR_ARG, "null pointer argument (out_off with out_mean, cov_off with out_cov)");
  STAGE(series_check_layout(c, sc));
  const size_t Q = S > 0 ? (size_t)sc.q_off[S] : 0;
  if ((int64_t)Q >= ((int64_t)1 << 31) || (Q > 0 && R > (((int64_t)1 << 31) - 1) / (int64_t)Q))
    return fail(c, AGP_ERR_ARG, "R * q_off[S] too large (2^31 or more)");
  const size_t nx = (size_t)R * Q;
  if (nx > 0 && !so.x) return fail(c, AGP_ERR_ARG, "null pointer argument (out_x)");
  if (R > 0 && !so.seeds && (!so.component || (!so.z && Q > 0))) return fail(c, AGP_ERR_ARG, "null pointer argument (seeds)");
  std::vector<double> tr(2 * (size_t)S);      // [slope (S) | intercept (S)]
  for (int32_t s = 0; s < S; ++s) {
    STAGE(series_check_joint(c, sc, s, "query"));
    STAGE(series_y_transform(c, s, so.y_slope, so.y_intercept, tr[(size_t)s], tr[(size_t)S + s]));
    if (so.z)
      for (long long k = 0, m = sc.q_off[s + 1] - sc.q_off[s]; k < R * m; ++k)
        if (!std::isfinite(so.z[R * sc.q_off[s] + k])) {
          snprintf(buf, sizeof buf, "series %d: z of sample %lld, point %lld is not finite", (int)s, k / m, k % m);
          return fail(c, AGP_ERR_ARG, buf);
        }
  }
  MixPlan qp;      // the mixtures' lists and weights (the transforms: checked above)
  STAGE(mix_plan(c, S, P, sc.series, sc.q_off, so.weights, nullptr, nullptr, 0, qp));
  const long long* pl_off = qp.pl_off();
  const long long* w_off = qp.w_off();
  // the component of every sample — the caller's, or drawn series by series as agp_predict_sample_batch draws under seeds[s] — and
  // from them every particle's list of samples (CSR, ascending)
  std::vector<int32_t> comp((size_t)S * (size_t)R), local;
  for (int32_t s = 0; s < S && R > 0; ++s) {
    const long long Ps = pl_off[s + 1] - pl_off[s];
    if (Ps == 0) {
      snprintf(buf, sizeof buf, "series %d has no particles to sample from", (int)s);
      return fail(c, AGP_ERR_ARG, buf);
    }
    int32_t* cs = comp.data() + (size_t)s * (size_t)R;
    if (so.component) {
      for (int64_t j = 0; j < R; ++j) {
        const int32_t g = so.component[(size_t)s * (size_t)R + (size_t)j];
        if (g < 0 || g >= P || sc.series[g] != s) {
          snprintf(buf, sizeof buf, "series %d: component %d of sample %lld is not a particle of the series", (int)s, (int)g, (long long)j);
          return fail(c, AGP_ERR_ARG, buf);
        }
        if (!(so.weights[g] > 0.0)) {
          snprintf(buf, sizeof buf, "series %d: component %d of sample %lld has weight 0", (int)s, (int)g, (long long)j);
          return fail(c, AGP_ERR_ARG, buf);
        }
        cs[j] = g;
      }
    } else {
      local.resize((size_t)R);
      draw_components(R, (int32_t)Ps, qp.vals.data() + w_off[s], so.seeds[s], local);
      for (int64_t j = 0; j < R; ++j) cs[j] = qp.plist[(size_t)(pl_off[s] + local[(size_t)j])];
    }
  }
  std::vector<long long> ltab(2 * ((size_t)P + 1), 0);      // [smp_off (P + 1) | cov_off (P + 1)]
  long long* smp_off = ltab.data();
  long long* cov_off = smp_off + P + 1;
  for (int32_t g : comp) ++smp_off[(size_t)g + 1];
  for (int p = 0; p < P; ++p) smp_off[p + 1] += smp_off[p];
  std::vector<int32_t> smp(comp.size());
  {
    std::vector<long long> at(smp_off, smp_off + P);
    for (int32_t s = 0; s < S; ++s)
      for (int64_t j = 0; j < R; ++j) smp[(size_t)at[(size_t)comp[(size_t)s * (size_t)R + (size_t)j]]++] = (int32_t)j;
  }
  STAGE(series_classes(c, sc, SeriesMode::held_out));
  for (int p = 0; p < P; ++p) cov_off[p + 1] = cov_off[p] + sc.nq[(size_t)p] * sc.nq[(size_t)p];
  // (no check is left to fail, nothing is launched yet)
  if (so.out_off) std::copy(sc.ooff.begin(), sc.ooff.end(), so.out_off);
  if (so.cov_off) std::copy(cov_off, cov_off + P + 1, so.cov_off);
  if (so.out_component) std::copy(comp.begin(), comp.end(), so.out_component);
  if (sc.wg.empty()) { series_zero_values(sc, nullptr, out_info); return AGP_OK; }      // no series has a query point: nothing to write
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  // sq_w = [slope (S) | intercept (S)]; sq_tab = [pl_off (S + 1) | seeds (S) | smp_off | cov_off (P + 1 each) | plist (P) | smp (S R)];
  // the samples in smp_x, the caller's normals in smp_zin, the components in pred_mean / pred_cov
  const size_t S1 = (size_t)S + 1, n_mean = so.mean ? sc.n_out() : 0, n_cov = so.cov ? (size_t)cov_off[P] : 0;
  const size_t o_seed = sizeof(long long) * S1, o_ltab = o_seed + sizeof(uint64_t) * (size_t)S,
               o_plist = o_ltab + sizeof(long long) * ltab.size(), o_smp = o_plist + sizeof(int32_t) * (size_t)P;
  const std::vector<uint64_t> seeds0((size_t)S, 0);
  HIPCHK(c, s->sq_w.ensure(sizeof(double) * tr.size()));
  HIPCHK(c, s->sq_tab.ensure(o_smp + sizeof(int32_t) * std::max<size_t>(1, smp.size())));
  HIPCHK(c, s->smp_x.ensure(sizeof(double) * std::max<size_t>(1, nx)));
  if (so.cov) HIPCHK(c, s->pred_cov.ensure(sizeof(double) * std::max<size_t>(1, n_cov)));
  sc.up.add(s->sq_w.p, tr.data(), sizeof(double) * tr.size());
  sc.up.add(s->sq_tab.p, pl_off, sizeof(long long) * S1);
  sc.up.add(s->sq_tab.as<char>() + o_seed, so.seeds ? so.seeds : seeds0.data(), sizeof(uint64_t) * (size_t)S);
  sc.up.add(s->sq_tab.as<char>() + o_ltab, ltab.data(), sizeof(long long) * ltab.size());
  sc.up.add(s->sq_tab.as<char>() + o_plist, qp.plist.data(), sizeof(int32_t) * (size_t)P);
  sc.up.add(s->sq_tab.as<char>() + o_smp, smp.data(), sizeof(int32_t) * smp.size());
  if (so.z && nx > 0) {
    HIPCHK(c, s->smp_zin.ensure(sizeof(double) * nx));
    sc.up.add(s->smp_zin.p, so.z, sizeof(double) * nx);
  }
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  SeriesSampleArgs pa = {};
  series_query_args(sc, pa);
  pa.y_slope = s->sq_w.as<double>(); pa.y_intercept = s->sq_w.as<double>() + S;
  pa.R = R;
  pa.seeds = reinterpret_cast<const unsigned long long*>(s->sq_tab.as<char>() + o_seed);
  pa.zin = so.z && nx > 0 ? s->smp_zin.as<double>() : nullptr;
  pa.smp_off = reinterpret_cast<const long long*>(s->sq_tab.as<char>() + o_ltab);
  pa.cov_off = pa.smp_off + P + 1;
  pa.smp = reinterpret_cast<const int32_t*>(s->sq_tab.as<char>() + o_smp);
  pa.out_x = s->smp_x.as<double>();
  pa.out_mean = so.mean ? s->pred_mean.as<double>() : nullptr;
  pa.out_cov = so.cov ? s->pred_cov.as<double>() : nullptr;
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    pa.wg = wg;
    return launch_series_predict_sample(sc.st, pa, grid, d == 0 ? 4 : 8, lds);
  }));
  if (nx > 0) {
    SeriesSampleFillArgs fa = {};
    fa.S = S; fa.R = R;
    fa.q_off = pa.q_off;
    fa.pl_off = s->sq_tab.as<long long>();
    fa.plist = reinterpret_cast<const int32_t*>(s->sq_tab.as<char>() + o_plist);
    fa.info = sc.sa.out_info;
    fa.out_x = pa.out_x;
    HIPCHK(c, launch_series_sample_fill(sc.st, fa));
  }
  STAGE(series_mark_readout(c, sc));
  // back: x (R q_off[S]), and mean (out_off[P]) and cov (cov_off[P]) when wanted (pred_cov exists only then: 0 bytes, never read)
  const int b_x = sc.want(s->smp_x.p, sizeof(double) * nx), b_mean = sc.want(s->pred_mean.p, sizeof(double) * n_mean),
            b_cov = sc.want(s->pred_cov.p, sizeof(double) * n_cov);
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, nullptr, out_info);      // (no query point: length 0 here, so info 0)
  // every series with query points has particles, every sample one of them as its component: the whole of x was written
  if (nx > 0) std::memcpy(so.x, sc.got<char>(b_x), sizeof(double) * nx);
  if (n_mean > 0) std::memcpy(so.mean, sc.got<char>(b_mean), sizeof(double) * n_mean);
  if (n_cov > 0) std::memcpy(so.cov, sc.got<char>(b_cov), sizeof(double) * n_cov);
  return series_timing(c, sc);
}

// The decomposition side of agp_predict_sum_series_batch: the components, transforms and quantiles, and the outputs beside [logpdf | info].
struct SeriesSumOut {
  int32_t M;                   // components per particle: particle p's are the CSR entries [p M, (p + 1) M) of the call's programs
  const double* y_slope;       // [S] or null (1)
  const double* y_intercept;   // [S] or null (0)
  const double* q; int64_t nq;
  double* mean; double* var;   // [out_off[P]]; var nullable
  double* x;                   // [nq out_off[P]]; unused when nq == 0
  int64_t* out_off;            // [P + 1]
};

// predict_sum's numbers of every particle on its own series: sc.pp arrives holding the P M COMPONENT programs; the composites
// K_1 SEL_1 * K_2 SEL_2 * + .. built from them take its place, and the stages run on those.  out_logpdf may be null.
int predict_sum_series(agp_ctx* c, SeriesCall& sc, const SeriesSumOut& so, double* out_logpdf, int32_t* out_info) {
  const int P = sc.pp.P;
  const int32_t S = sc.S, M = so.M;
  const int64_t nq = so.nq;
  char buf[256];
  STAGE(series_check_sizes(c, sc));
  if (M < 1) return fail(c, AGP_ERR_ARG, "M must be >= 1 (components per particle)");
  if (nq < 0) return fail(c, AGP_ERR_ARG, "negative size (nq)");
  if (nq > 0 && !so.q) return fail(c, AGP_ERR_ARG, "null q");
  for (int64_t k = 0; k < nq; ++k)
    if (!(so.q[k] > 0.0 && so.q[k] < 1.0)) {
      snprintf(buf, sizeof buf, "quantile %lld must be in (0, 1)", (long long)k);
      return fail(c, AGP_ERR_ARG, buf);
    }
  if (P == 0) return AGP_OK;
  STAGE(series_check_pointers(c, sc, out_info != nullptr));
  if (!sc.q_off || !sc.ts_pred || !so.mean || !so.out_off || (nq > 0 && !so.x))
    return fail(c, AGP_ERR_ARG, "null pointer argument (q_off, ts_pred, out_mean, out_off, or out_x with quantiles asked)");
  if ((int64_t)P * M >= ((int64_t)1 << 31)) return fail(c, AGP_ERR_ARG, "P * M too large");
  // the composite programs, particle by particle (as agp_infer_gp_sum_batch)
  const Particles comp = sc.pp;
  std::vector<int32_t> coff((size_t)P + 1, 0), cpoff((size_t)P + 1, 0);
  std::vector<uint8_t> cops; std::vector<double> cprm;
  std::string err;
  for (int p = 0; p < P; ++p) {
    if (const int rc = append_composite(comp, (int64_t)p * M, M, AGP_MAX_OPS, cops, cprm, err)) {
      snprintf(buf, sizeof buf, "particle %d: ", p);
      return fail(c, rc, buf + err);
    }
    coff[(size_t)p + 1] = (int32_t)cops.size(); cpoff[(size_t)p + 1] = (int32_t)cprm.size();
  }
  sc.pp = {P, coff.data(), cops.data(), cpoff.data(), cprm.data(), comp.noise, comp.noise_pred};
  STAGE(series_check_layout(c, sc));
  std::vector<double> vals(2 * (size_t)S + (size_t)nq);      // [slope (S) | intercept (S) | z (nq)]
  for (int32_t s = 0; s < S; ++s) STAGE(series_y_transform(c, s, so.y_slope, so.y_intercept, vals[(size_t)s], vals[(size_t)S + s]));
  for (int64_t k = 0; k < nq; ++k) vals[2 * (size_t)S + (size_t)k] = ndtri(so.q[k]);
  {
    int64_t rows = 0;      // (M + 1) sum_p m_{series[p]}: m_s <= 2^30 and M < 2^31, so every step stays far inside int64
    const int64_t lim = (int64_t)1 << 31;
    for (int p = 0; p < P; ++p) {
      rows += ((int64_t)M + 1) * (sc.q_off[sc.series[p] + 1] - sc.q_off[sc.series[p]]);
      if (rows >= lim || (nq > 0 && rows >= lim / nq)) {
        snprintf(buf, sizeof buf, "particle %d: an output reaches 2^31 elements", p);
        return fail(c, AGP_ERR_ARG, buf);
      }
    }
  }
  STAGE(series_classes(c, sc, SeriesMode::sum));
  for (long long& o : sc.ooff) o *= (long long)M + 1;      // out_off counts rows: M + 1 per query point
  std::copy(sc.ooff.begin(), sc.ooff.end(), so.out_off);   // (no check is left to fail, nothing is launched yet)
  if (sc.wg.empty()) { series_zero_values(sc, out_logpdf, out_info); return AGP_OK; }
  STAGE(series_stage(c, sc));
  Slot* s = sc.s;
  // sq_w = [slope (S) | intercept (S) | z (nq)]; the raw marginals in pred_mean / pred_var, the quantiles in sum_x
  const size_t n_out = sc.n_out(), nx = n_out * (size_t)nq;
  HIPCHK(c, s->sq_w.ensure(sizeof(double) * std::max<size_t>(1, vals.size())));
  HIPCHK(c, s->sum_x.ensure(sizeof(double) * std::max<size_t>(1, nx)));
  sc.up.add(s->sq_w.p, vals.data(), sizeof(double) * vals.size());
  HIPCHK(c, sc.up.flush(s->h_stage, s->up_blob, sc.st));
  SeriesSumArgs pa = {};
  series_query_args(sc, pa);
  pa.out_mean = s->pred_mean.as<double>(); pa.out_var = s->pred_var.as<double>();
  pa.M = M; pa.nq = (int)nq;
  pa.y_slope = s->sq_w.as<double>(); pa.y_intercept = pa.y_slope + S; pa.z = pa.y_intercept + S;
  pa.out_x = s->sum_x.as<double>();
  STAGE(series_launch(c, sc, [&](const int32_t* wg, int grid, int d, size_t lds) {
    pa.wg = wg;
    return launch_series_predict_sum(sc.st, pa, grid, d == 0 ? 4 : 8, lds);
  }));
  const int b_mean = sc.want(s->pred_mean.p, sizeof(double) * n_out), b_var = sc.want(s->pred_var.p, sizeof(double) * n_out),
            b_x = sc.want(s->sum_x.p, sizeof(double) * nx);
  STAGE(series_fetch(c, sc));
  series_copy_values(sc, out_logpdf, out_info);
  // (an empty series with query points was launched for its prior: its value is 0, but a row without a raw marginal still reports)
  const int32_t* hi = reinterpret_cast<const int32_t*>(static_cast<const double*>(s->h_out.p) + P);
  for (int p = 0; p < P; ++p)
    if (sc.len[(size_t)p] == 0 && sc.nq[(size_t)p] > 0) out_info[p] = hi[p];
  if (n_out > 0) {      // every particle with query points was launched and wrote its whole blocks
    std::memcpy(so.mean, sc.got<char>(b_mean), sizeof(double) * n_out);
    if (so.var) std::memcpy(so.var, sc.got<char>(b_var), sizeof(double) * n_out);
  }
  if (nx > 0) std::memcpy(so.x, sc.got<char>(b_x), sizeof(double) * nx);
  return series_timing(c, sc);
}

#undef STAGE

// The packed blocks (bel doubles per matrix) and padded alpha (np per matrix) of the two factor probes -> row-major L with zeros above
// the diagonal, and alpha: element (r, col) of block (rb, cb) sits at col * 16 + r of block rb (rb + 1) / 2 + cb (blk_idx).
void series_unpack_factor(const double* blk, const double* av, int64_t n, int32_t P, int np, size_t bel, double* out_L, double* out_alpha) {
  const size_t nel = (size_t)n * n;
  for (int p = 0; p < P; ++p) {
    const double* b = blk + (size_t)p * bel;
    double* L = out_L + (size_t)p * nel;
    for (int64_t r = 0; r < n; ++r)
      for (int64_t col = 0; col < n; ++col) {
        const size_t at = ((size_t)(r / 16) * (r / 16 + 1) / 2 + (size_t)(col / 16)) * 256 + (size_t)(col % 16) * 16 + (size_t)(r % 16);
        L[r * n + col] = col <= r ? b[at] : 0.0;
      }
    std::copy(av + (size_t)p * np, av + (size_t)p * np + n, out_alpha + (size_t)p * n);
  }
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
  series_unpack_factor(blk.data(), av.data(), n, P, m.np, bel, out_L, out_alpha);
  return AGP_OK;
}

// agp_debug_long_series_factor: P caller matrices of one size through stage 3 (b) - (e) and stage 4 of the long-series value kernel
// (its probe instantiation); the workspace the kernel factors in is read back and unpacked as above.
int long_series_factor(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, double* out_L, double* out_alpha,
                       double* out_part, double* out_lp, int32_t* out_info) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (n <= 0 || n > AGP_LONG_SERIES_MAX_N) {
    char buf[128];
    snprintf(buf, sizeof buf, "long-series probe: n = %lld outside [1, AGP_LONG_SERIES_MAX_N = %d]", (long long)n, AGP_LONG_SERIES_MAX_N);
    return fail(c, AGP_ERR_ARG, buf);
  }
  if (P <= 0 || P > 256) return fail(c, AGP_ERR_ARG, "long-series probe: 1 .. 256 matrices per call");
  if (!K || !out_L || !out_alpha || !out_part || !out_lp || !out_info) return fail(c, AGP_ERR_ARG, "null pointer argument");
  const LongSeriesLds m = long_series_lds((int)n, 0, 0, 0);
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
  LongSeriesProbeArgs la = {};
  la.K = s->dense.as<double>(); la.y = y ? s->vec.as<double>() : nullptr; la.n = (int)n;
  la.ws = s->A.as<double>(); la.ws_stride = (long long)bel;
  la.out_alpha = s->alpha.as<double>(); la.out_part = s->partial.as<double>();
  la.out_lp = s->out_lp.as<double>(); la.out_info = reinterpret_cast<int32_t*>(s->out_lp.as<double>() + P);
  HIPCHK(c, launch_long_series_probe(st, la, P, sizeof(double) * (size_t)m.total));
  std::vector<double> blk(bel * P), av((size_t)m.np * P);
  HIPCHK(c, hipMemcpyAsync(blk.data(), s->A.p, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(av.data(), s->alpha.p, sizeof(double) * av.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_part, s->partial.p, sizeof(double) * 2 * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_lp, s->out_lp.p, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_info, la.out_info, sizeof(int32_t) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  series_unpack_factor(blk.data(), av.data(), n, P, m.np, bel, out_L, out_alpha);
  return AGP_OK;
}

// what the long entries share: the cap, its name, and the flags (AGP_LONG_SERIES_ALL is the only bit)
int series_long_entry(agp_ctx* c, SeriesCall& sc, uint32_t flags) {
  sc.max_n = AGP_LONG_SERIES_MAX_N; sc.max_name = "AGP_LONG_SERIES_MAX_N";
  sc.all_long = (flags & AGP_LONG_SERIES_ALL) != 0;
  if (c && (flags & ~(uint32_t)AGP_LONG_SERIES_ALL) != 0) {
    char buf[96];
    snprintf(buf, sizeof buf, "unknown flag bits 0x%x (AGP_LONG_SERIES_ALL is the only flag)", (unsigned)(flags & ~(uint32_t)AGP_LONG_SERIES_ALL));
    return fail(c, AGP_ERR_ARG, buf);
  }
  return AGP_OK;
}

}  // namespace

extern "C" {

int agp_logpdf_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P,
                            const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                            const double* noise, double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, nullptr}, series, nullptr, nullptr};
    return logpdf_series(c, sc, out_logpdf, out_info);
  });
}

int agp_logpdf_long_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P,
                                 const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                 const double* noise, int32_t flags, double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, nullptr}, series, nullptr, nullptr};
    if (const int rc = series_long_entry(c, sc, (uint32_t)flags)) return rc;
    return logpdf_series(c, sc, out_logpdf, out_info, SeriesMode::long_value);
  });
}

int agp_predict_long_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, const int64_t* q_off,
                                  const double* ts_pred, int32_t P, const int32_t* series, const int32_t* op_off, const uint8_t* ops,
                                  const int32_t* prm_off, const double* prm, const double* noise, const double* noise_pred,
                                  double* out_mean, double* out_var, int64_t* out_off, double* out_logpdf, int32_t* out_info,
                                  uint32_t flags) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    if (const int rc = series_long_entry(c, sc, flags)) return rc;
    sc.ws_blocks = long_series_pred_ws_blocks;
    return predict_series(c, sc, out_mean, out_var, out_off, out_logpdf, out_info, SeriesMode::long_prediction);
  });
}

int agp_predict_quantile_long_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs,
                                           const int64_t* q_off, const double* ts_pred, int32_t P, const int32_t* series,
                                           const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                           const double* noise, const double* noise_pred, const double* weights, const double* y_slope,
                                           const double* y_intercept, const double* q, int64_t nq, double tol, int64_t max_iter,
                                           double* out_x, int32_t* out_converged, int32_t* out_iters, double* out_mix_mean,
                                           double* out_mix_var, double* out_logpdf, int32_t* out_info, uint32_t flags) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesQuantOut qo{weights, y_slope, y_intercept, q, nq, tol, max_iter, out_x, out_converged, out_iters, out_mix_mean, out_mix_var};
    if (const int rc = series_long_entry(c, sc, flags)) return rc;
    sc.ws_blocks = long_series_pred_ws_blocks;
    return predict_quantile_series(c, sc, qo, out_logpdf, out_info, SeriesMode::long_prediction);
  });
}

int agp_logpdf_grad_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P,
                                 const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                 const double* noise, double* out_logpdf, double* out_grad, double* out_grad_noise, int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, nullptr}, series, nullptr, nullptr};
    return logpdf_grad_series(c, sc, out_logpdf, out_grad, out_grad_noise, out_info);
  });
}

int agp_predict_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, const int64_t* q_off,
                             const double* ts_pred, int32_t P, const int32_t* series, const int32_t* op_off, const uint8_t* ops,
                             const int32_t* prm_off, const double* prm, const double* noise, const double* noise_pred, double* out_mean,
                             double* out_var, int64_t* out_off, double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    return predict_series(c, sc, out_mean, out_var, out_off, out_logpdf, out_info);
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
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesQuantOut qo{weights, y_slope, y_intercept, q, nq, tol, max_iter, out_x, out_converged, out_iters, out_mix_mean, out_mix_var};
    return predict_quantile_series(c, sc, qo, out_logpdf, out_info);
  });
}

int agp_predict_logpdf_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs,
                                    const int64_t* q_off, const double* ts_pred, const double* y_pred, int32_t P, const int32_t* series,
                                    const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                                    const double* noise, const double* noise_pred, const double* y_slope, const double* weights,
                                    double* out_logpdf, double* out_terms, int64_t* out_off, double* out_series_logp, int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesProbaOut po{y_pred, y_slope, weights, out_terms, out_off, out_series_logp};
    return predict_logpdf_series(c, sc, po, out_logpdf, out_info);
  });
}

int agp_predict_logpdf_long_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs,
                                         const int64_t* q_off, const double* ts_pred, const double* y_pred, int32_t P,
                                         const int32_t* series, const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off,
                                         const double* prm, const double* noise, const double* noise_pred, const double* y_slope,
                                         const double* weights, double* out_logpdf, double* out_terms, int64_t* out_off,
                                         double* out_series_logp, int32_t* out_info, uint32_t flags) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesProbaOut po{y_pred, y_slope, weights, out_terms, out_off, out_series_logp};
    if (const int rc = series_long_entry(c, sc, flags)) return rc;
    return predict_logpdf_series(c, sc, po, out_logpdf, out_info, SeriesMode::long_held_out);
  });
}

int agp_predict_sample_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs,
                                    const int64_t* q_off, const double* ts_pred, int32_t P, const int32_t* series, const int32_t* op_off,
                                    const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                                    const double* noise_pred, const double* y_slope, const double* y_intercept, const double* weights,
                                    int64_t R, const uint64_t* seeds, const int32_t* component, const double* z, double* out_x,
                                    int32_t* out_component, double* out_mean, int64_t* out_off, double* out_cov, int64_t* cov_off,
                                    int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesSampleOut so{y_slope, y_intercept, weights, R, seeds, component, z, out_x, out_component, out_mean, out_off, out_cov, cov_off};
    return predict_sample_series(c, sc, so, out_info);
  });
}

int agp_predict_sum_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, const int64_t* q_off,
                                 const double* ts_pred, int32_t P, int32_t M, const int32_t* series, const int32_t* op_off,
                                 const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                                 const double* noise_pred, const double* y_slope, const double* y_intercept, const double* q, int64_t nq,
                                 double* out_mean, double* out_var, double* out_x, int64_t* out_off, double* out_logpdf,
                                 int32_t* out_info) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, prm, noise, noise_pred}, series, q_off, ts_pred};
    const SeriesSumOut so{M, y_slope, y_intercept, q, nq, out_mean, out_var, out_x, out_off};
    return predict_sum_series(c, sc, so, out_logpdf, out_info);
  });
}

int agp_hmc_series_batch(agp_ctx* c, int32_t S, const int64_t* pt_off, const double* ts, const double* xs, int32_t P, const int32_t* series,
                         const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* z, const double* z_noise,
                         const int32_t* prm_class, int32_t C, const double* tf, int32_t noise_class, double noise_jitter, int32_t n_hmc,
                         int32_t L_param, double eps_param, int32_t L_noise, double eps_noise, int32_t n_exit, const uint64_t* seeds,
                         int32_t flags, double* out_z, double* out_z_noise, double* out_prm, double* out_noise, double* out_logpdf,
                         int32_t* out_counts, int32_t* out_info, double* out_trace) {
  return abi_guard(c, [&] {
    SeriesCall sc{S, pt_off, ts, xs, {P, op_off, ops, prm_off, nullptr, nullptr, nullptr}, series, nullptr, nullptr};
    const SeriesHmcCall hm{z, z_noise, prm_class, C, tf, noise_class, noise_jitter, n_hmc, L_param, eps_param, L_noise, eps_noise, n_exit,
                           seeds, flags, out_z, out_z_noise, out_prm, out_noise, out_counts, out_trace};
    return hmc_series(c, sc, hm, out_logpdf, out_info);
  });
}

int agp_debug_series_factor(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, double* out_L, double* out_alpha,
                            double* out_partial, double* out_lp, int32_t* out_info) {
  return abi_guard(c, [&] { return series_factor(c, K, y, n, P, out_L, out_alpha, out_partial, out_lp, out_info); });
}

int agp_debug_long_series_factor(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, double* out_L, double* out_alpha,
                                 double* out_partial, double* out_lp, int32_t* out_info) {
  return abi_guard(c, [&] { return long_series_factor(c, K, y, n, P, out_L, out_alpha, out_partial, out_lp, out_info); });
}

}  // extern "C"
