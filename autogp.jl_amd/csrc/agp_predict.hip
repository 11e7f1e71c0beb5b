// Host side of the C ABI, unit 2: predictive entries (src/GP.jl:731-758, 904-993), matrix assembly and the probe entries.
// The dense predictive pass (predict_core, predict_logpdf_core) is written as stages over one JointPlan: see the list above split_queries.
#include "agp_host.hpp"
#include "agp_ndtri.hpp"
#ifdef AGP_EXPERIMENTS
#include "experiments/agp_experiments_abi.h"
#include "experiments/agp_experiments.hpp"   // ablation kernels of the update GEMM (measurement builds only: libautogp_hip_exp.so)
#endif


#ifdef AGP_EXPERIMENTS
template <int VAR>
static void launch_variant(hipStream_t st, int grid, const CholArgs& ca) {
  hipLaunchKernelGGL(k_gemm_variant<VAR>, dim3(grid), dim3(256), 0, st, ca);
}
#endif
namespace {

// Query points on the series' own lattice.  In every use of the reference the query set is `train + test + future` at the
// data's cadence (scripts/online.jl:41-43: ds_query = vcat(model.ds, ds_next, ds_test); src/GP.jl:743 evaluates the kernel on
// [ts; ts_pred]): on a regular grid every joint point then has an integer RANK round((t - t_0) / h) — duplicates of training
// times share one, future points exceed n_max - 1, earlier ones are negative — and |t_a - t_b| = |rank_a - rank_b| h for every
// pair of the joint set: the stationary subtrees of the predictive pass read the same rank tables as the factor store's sweeps,
// extended to max rank - min rank + 1 lags.  One off-lattice point (same tolerance as agp_set_data) -> general path.
struct PredLattice {
  bool on = false;
  int R = 0, rank_units = 1;
  std::vector<int32_t> rank;      // joint padded layout [ts(1:n), pad, ts_pred, pad], shifted so that the smallest rank is 0
  std::vector<double> tl;         // time of lag g: t_sorted[g] inside the data (the store's tables), t_0 + g h beyond
};
constexpr int64_t PRED_MAX_LAGS = LAG_LDS_MAX_UNITS * 256;     // (LDS capacity of the fused evaluators, as for the resident series)

void predict_lattice(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, PredLattice& pl) {
  pl.on = false;
  if (!(c->lag_ok && c->lag_enable && c->lag_rank_enable) || n <= 0 || m <= 0 || c->h_rank.empty()) return;
  const double t0 = c->h_ts_sorted.front(), h = c->grid_h;
  const int n1_pad = round_up(n, NB), m_pad = round_up(m, NB);
  std::vector<long long> gq((size_t)m);
  long long gmin = 0, gmax = (long long)c->n_lat - 1;
  for (int64_t j = 0; j < m; ++j) {
    const double t = ts_pred[j];
    const double gf = std::nearbyint((t - t0) / h);
    if (!std::isfinite(gf) || std::fabs(gf) > 1e6) return;
    const double tol = c->lat_tol_abs - 2.220446049250313e-16 * std::max(std::fabs(t), std::max(std::fabs(t0), std::fabs(c->h_ts_sorted.back())));
    if (!(tol > 0.0) || std::fabs(t - (t0 + gf * h)) > tol) return;
    gq[(size_t)j] = (long long)gf;
    gmin = std::min(gmin, gq[(size_t)j]); gmax = std::max(gmax, gq[(size_t)j]);
  }
  const long long R = gmax - gmin + 1;
  // (tables beyond the fused evaluators' LDS would be gathered from L2 in the caller's order, which is slower than evaluating the
  // leaves: measured 41.1 vs 39.5 ms on 2048 month starts — such a call takes the general evaluator; see logpdf_batch_impl)
  if (R > PRED_MAX_LAGS) return;
  pl.R = (int)R; pl.rank_units = (int)((R + 255) / 256);
  pl.rank.assign((size_t)n1_pad + m_pad, 0);
  for (int64_t i = 0; i < n; ++i) pl.rank[(size_t)i] = (int32_t)(c->h_rank[(size_t)i] - gmin);
  for (int64_t j = 0; j < m; ++j) pl.rank[(size_t)n1_pad + j] = (int32_t)(gq[(size_t)j] - gmin);
  pl.tl.assign((size_t)pl.rank_units * 256, 0.0);
  for (long long g = 0; g < (long long)pl.tl.size(); ++g)
    pl.tl[(size_t)g] = g < c->n_lat ? c->h_ts_lat[(size_t)g] : (c->lag_contig ? t0 + (double)g * h : (double)g * h);      // (lattice with gaps: exact lags, see agp_set_data)
  pl.on = true;
}

// ---- the dense predictive pass, stage by stage --------------------------------------------------------------------------------------
//   plan_joint        the joint matrix, planned once per call: which queries it keeps (split_queries), its points, its tile geometry
//   ResidentFactors   store lookup, the store's lock, the resident Z = L^-T of the training-point route
//   size_buffers, stage_joint, stage_modes, flush_uploads          buffer sizes and the one flush of every upload
//   per chunk: landing_zone, chunk_setup + launch_cov (tiles), the factorisation, z_chain, launch_schur, extract_chunk,
//              sum_readout_chunk / mix_chunk, the copy-back, scatter_chunk
//   finish_info       the info pass after the last chunk
// predict_core lists them top to bottom; predict_logpdf_core shares the plan, stage_joint, flush_uploads and chunk_setup.

// Query points that are training points (see JointPlan): positions in ts_pred + training indices, and the other queries.
// Empty lists when the shortcut does not apply or would not pay.
void split_queries(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, bool eligible,
                   std::vector<int32_t>& dq, std::vector<int32_t>& di, std::vector<int32_t>& fq) {
  dq.clear(); di.clear(); fq.clear();
  if (!eligible || n < 2 * NB || m < NB) return;
  auto bits = [](double x) { if (x == 0.0) x = 0.0; uint64_t u; std::memcpy(&u, &x, 8); return u; };
  std::unordered_map<uint64_t, int32_t> at;
  at.reserve((size_t)n * 2);
  for (int64_t i = 0; i < n; ++i) at.emplace(bits(c->h_ts[(size_t)i]), (int32_t)i);
  for (int64_t j = 0; j < m; ++j) {
    auto it = ts_pred[j] == ts_pred[j] ? at.find(bits(ts_pred[j])) : at.end();
    if (it != at.end()) { dq.push_back((int32_t)j); di.push_back(it->second); }
    else fq.push_back((int32_t)j);
  }
  // (worth it once the duplicates' share of V costs more than the n^3/3 of Z)
  if ((int64_t)dq.size() * 3 < n || (int64_t)dq.size() < NB) { dq.clear(); di.clear(); fq.clear(); }
}

// The joint matrix [K11 + noise I, K12; K21, K22] of a dense pass, planned ONCE per call: the entry makes the plan before it compiles
// the batch (use_flow and the compile options see the nt, nt1 that will run) and hands the same plan to the pass.
// ---- query points that ARE training points, no covariance requested, no codes (diag_path) ------------------------------------------
// For t*_j == t_i the cross-covariance row is K21[j,:] = K11[i,:] - noise e_i^T (src/GP.jl:743-747 evaluates the kernel
// on the joint list; the noise sits on K11's diagonal only), so with alpha = K11^-1 (y - mu1):
//     mean*_j = mu2_j + (y - mu1)_i - noise alpha_i,      var*_j = noise - noise^2 (K11^-1)_ii + noise_pred,
// and (K11^-1)_ii = sum_c Z(i,c)^2 with Z = L^-T: k_trtri_chain forms Z and alpha in n^3/3 flops per particle where the
// joint path spends n^2 flops PER SUCH POINT on V = L^-1 K12 (the reference's query set is train + test + future,
// scripts/online.jl:41-43: n of its points are of this kind).  The other query points (fq) stay in the joint matrix.
struct JointPlan {
  PredQuery q = {};                        // the caller's query
  bool want_cov = false, has_codes = false;
  const PredLattice* pl = nullptr;         // the query's lattice (null or off: the general evaluators)
  std::vector<int32_t> dq, di, fq;         // duplicates: position in ts_pred, training index; the remaining queries
  bool diag_path = false;                  // the split is taken
  int64_t mJ = 0;                          // query points of the joint matrix
  const double* tsJ = nullptr; const double* meanJ = nullptr; const double* daddJ = nullptr;      // per joint query point (nullable as given)
  int n1_pad = 0, m_pad = 0, nt1 = 0, nt2 = 0, nt = 0, ntot = 0, ntiles = 0;      // (n1_pad: 0 when n == 0)
  long long strideA = 0, strideZ = 0;      // per particle: the joint tiles; Z = L11^-T (training tiles only, diag_path)
  std::vector<double> tsF, meanF, daddF;   // (the filtered lists tsJ / meanJ / daddJ point into)
  std::vector<int32_t> rankF;              // (the joint layout keeps the ranks of the queries that are not training points only)
  JointPlan() = default;
  JointPlan(const JointPlan&) = delete; JointPlan& operator=(const JointPlan&) = delete;
  bool lagr() const { return pl != nullptr && pl->on; }
  const std::vector<int32_t>& rank() const { return diag_path ? rankF : pl->rank; }      // lattice ranks, padded joint layout (lagr() only)
  int chunk(agp_ctx* c, int P) const { return (int)std::max<int64_t>(1, std::min<int64_t>(P, ws_limit_bytes(c) / ((strideA + strideZ) * 8))); }
};

// `diag_add` (nullable, per query point) is filtered with the split; a pass that forms whole covariances (want_cov) or has coded
// query points never splits.
void plan_joint(agp_ctx* c, const PredQuery& q, bool want_cov, bool has_codes, const double* diag_add, const PredLattice* pl, JointPlan& jp) {
  const int64_t n = q.n, m = q.m;
  jp.q = q; jp.want_cov = want_cov; jp.has_codes = has_codes; jp.pl = pl;
  split_queries(c, n, q.ts_pred, m, !want_cov && !has_codes && !c->ref_arith, jp.dq, jp.di, jp.fq);
  jp.diag_path = !jp.dq.empty();
  const int64_t mJ = jp.mJ = jp.diag_path ? (int64_t)jp.fq.size() : m;
  jp.tsJ = q.ts_pred; jp.meanJ = q.mean_pred; jp.daddJ = diag_add;
  if (jp.diag_path) {
    const std::vector<int32_t>& fq = jp.fq;
    auto keep = [&](const double* v, std::vector<double>& f) { f.resize((size_t)mJ); for (int64_t g = 0; g < mJ; ++g) f[(size_t)g] = v[fq[(size_t)g]]; return f.data(); };
    jp.tsJ = keep(q.ts_pred, jp.tsF);
    if (q.mean_pred) jp.meanJ = keep(q.mean_pred, jp.meanF);
    if (diag_add) jp.daddJ = keep(diag_add, jp.daddF);
  }
  jp.n1_pad = round_up(n, NB); jp.m_pad = round_up(mJ, NB);
  jp.nt1 = jp.n1_pad / NB; jp.nt2 = jp.m_pad / NB; jp.nt = jp.nt1 + jp.nt2;
  jp.ntot = jp.n1_pad + jp.m_pad;
  jp.ntiles = jp.nt * (jp.nt + 1) / 2;
  jp.strideA = (long long)jp.ntiles * NB2;
  jp.strideZ = jp.diag_path ? (long long)(jp.nt1 * (jp.nt1 + 1) / 2) * NB2 : 0;
  if (jp.diag_path && jp.lagr()) {
    jp.rankF.assign((size_t)jp.ntot, 0);
    std::copy(pl->rank.begin(), pl->rank.begin() + jp.n1_pad, jp.rankF.begin());
    for (int64_t g = 0; g < mJ; ++g) jp.rankF[(size_t)jp.n1_pad + g] = pl->rank[(size_t)jp.n1_pad + jp.fq[(size_t)g]];
  }
}

struct SortedNoise { std::vector<double> noise, pred; };      // per sorted position (noise_pred defaults to noise)

// What predict_core and predict_logpdf_core stage alike for a compiled batch: the joint point list [ts(1:n), pad, tsJ(1:mJ), pad], the
// programs, the noises in sorted order, the means of the training and of the query points; and the buffers both size alike for
// chunks of `chunk` particles.
int stage_joint(agp_ctx* c, Slot* s, PinnedUploads& up, const JointPlan& jp, const Particles& pp, const Batch& bt, int chunk, SortedNoise& nz) {
  const int64_t n = jp.q.n, mJ = jp.mJ;
  const int P = pp.P;
  const int ntot = jp.ntot, nt = jp.nt;
  std::vector<double> tt((size_t)ntot, 0.0);
  std::copy(c->h_ts.begin(), c->h_ts.begin() + n, tt.begin());
  std::copy(jp.tsJ, jp.tsJ + mJ, tt.begin() + jp.n1_pad);
  nz.noise.resize((size_t)P); nz.pred.resize((size_t)P);
  for (int q = 0; q < P; ++q) {
    const int p = bt.order[q];
    nz.noise[q] = pp.noise[p];
    nz.pred[q] = pp.noise_pred ? pp.noise_pred[p] : pp.noise[p];
  }
  HIPCHK(c, s->vec.ensure(sizeof(double) * (size_t)ntot * chunk));
  HIPCHK(c, s->partial.ensure(sizeof(double) * 2 * (size_t)nt * chunk));
  HIPCHK(c, s->info.ensure(sizeof(int) * (size_t)P));
  HIPCHK(c, s->ready.ensure(sizeof(int) * (size_t)P));
  HIPCHK(c, s->hdr.ensure(sizeof(ProgHdr) * (size_t)P));
  HIPCHK(c, s->ops.ensure(bt.ops.size()));
  HIPCHK(c, s->prm.ensure(sizeof(double) * std::max<size_t>(1, bt.prm.size())));
  HIPCHK(c, s->noise.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->noise_pred.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->tt.ensure(sizeof(double) * (size_t)ntot));
  if (jp.q.mean_train && n > 0) {
    HIPCHK(c, s->mu1.ensure(sizeof(double) * (size_t)n));
    up.add(s->mu1.p, jp.q.mean_train, sizeof(double) * n);
  }
  if (jp.meanJ && mJ > 0) {
    HIPCHK(c, s->mu2.ensure(sizeof(double) * (size_t)mJ));
    up.add(s->mu2.p, jp.meanJ, sizeof(double) * mJ);
  }
  up.add(s->hdr.p, bt.hdr.data(), sizeof(ProgHdr) * P);
  up.add(s->ops.p, bt.ops.data(), bt.ops.size());
  up.add(s->prm.p, bt.prm.data(), sizeof(double) * bt.prm.size());
  up.add(s->noise.p, nz.noise.data(), sizeof(double) * P);
  up.add(s->noise_pred.p, nz.pred.data(), sizeof(double) * P);
  up.add(s->tt.p, tt.data(), sizeof(double) * ntot);
  return AGP_OK;
}

// The one flush of a pass's uploads.  Query points on the lattice: `up` goes out with the ranks of the joint points (padded joint
// layout), the lag times and the table programs; then one rank table of R lags per stationary subtree of the batch.
int flush_uploads(agp_ctx* c, Slot* s, hipStream_t st, PinnedUploads& up, const Batch& bt, const JointPlan& jp) {
  if (!jp.lagr()) {
    HIPCHK(c, up.flush(s->h_stage, s->up_blob, st));
    return AGP_OK;
  }
  const PredLattice& pl = *jp.pl;
  const std::vector<int32_t>& rank = jp.rank();
  const LagProgLayout lpl(bt);
  HIPCHK(c, lpl.upload(up, s->pl_prog));
  HIPCHK(c, s->pl_rank.ensure(sizeof(int32_t) * rank.size()));
  HIPCHK(c, s->pl_tl.ensure(sizeof(double) * pl.tl.size()));
  up.add(s->pl_rank.p, rank.data(), sizeof(int32_t) * rank.size());
  up.add(s->pl_tl.p, pl.tl.data(), sizeof(double) * pl.tl.size());
  HIPCHK(c, up.flush(s->h_stage, s->up_blob, st));
  if (bt.n_lag_tables > 0) {
    HIPCHK(c, s->lagtab.ensure(sizeof(double) * (size_t)bt.n_lag_tables * pl.rank_units * 256));
    LagArgs la = {};
    la.tt = s->pl_tl.as<double>(); la.tab = s->lagtab.as<double>();
    lpl.point(la, s->pl_prog.p);
    la.nt = 2 * pl.rank_units; la.full = 1; la.stride = pl.rank_units * 256;      // (every entry of the table is live)
    launch_lag_tables(st, la, pl.rank_units, bt.n_lag_tables);
    HIPCHK(c, hipGetLastError());
  }
  std::lock_guard<std::mutex> g(c->mu);
  ++c->n_lag_pred;
  return AGP_OK;
}

// CovArgs / CholArgs of sorted positions [p0, p0 + Pc) of a pass over the plan's joint matrix, and the chunk's share of fused
// particles (nf of them, evaluator depth dcov).  What differs between the passes is left to the caller, on cv and ca alike where both
// have the field: code, noise_q, i0; cv.skip_pred_offdiag; ca.nt1 (here: the training block), ca.wsteps.
struct JointChunk { CovArgs cv; CholArgs ca; int nf, dcov; };
JointChunk chunk_setup(Slot* s, const JointPlan& jp, const Batch& bt, int p0, int Pc) {
  JointChunk k = {};
  CovArgs& cv = k.cv;
  cv.tt = s->tt.as<double>(); cv.n1 = (int)jp.q.n; cv.n1_pad = jp.n1_pad; cv.m2 = (int)jp.mJ; cv.nt = jp.nt;
  cv.hdr = s->hdr.as<ProgHdr>() + p0; cv.ops = s->ops.as<uint8_t>(); cv.prm = s->prm.as<double>();
  cv.noise = s->noise.as<double>() + p0; cv.A = s->A.as<double>(); cv.strideA = jp.strideA; cv.P = Pc;
  if (jp.lagr()) { cv.lagtab = s->lagtab.as<double>(); cv.lagr = s->pl_rank.as<int32_t>(); cv.lag_stride = jp.pl->rank_units * 256; }
  k.nf = std::max(0, std::min(Pc, bt.n_fused - p0));
  k.dcov = k.nf > 0 ? bt.max_depth_fused : 0;
  cv.p_off = k.nf;
  CholArgs& ca = k.ca;
  ca.A = s->A.as<double>(); ca.strideA = jp.strideA; ca.W = s->W.as<double>();
  ca.vec = s->vec.as<double>(); ca.ldv = jp.ntot; ca.partial = s->partial.as<double>();
  ca.info = s->info.as<int>() + p0; ca.P = Pc; ca.nt = jp.nt; ca.k = 0; ca.nt1 = jp.nt1;
  set_cov(ca, cv);
  ca.lag = jp.lagr() ? 1 : 0;
  ca.n_fused = k.nf;
  ca.ready = s->ready.as<int>() + p0;
  return k;
}

// The dataflow schedule over the joint matrix of ca.P particles: block columns [0, wsteps) factored, every row of them (tile rows below
// ca.i0[p], when given, hold a resident factor already).
int launch_joint_flow(agp_ctx* c, Slot* s, hipStream_t st, CholArgs& ca, int dcov, int wsteps) {
  const int ntri = ca.nt * (ca.nt + 1) / 2;
  HIPCHK(c, s->tflag.ensure(sizeof(int) * (size_t)ca.P * ntri));
  HIPCHK(c, s->flowq.ensure(sizeof(int) * 8 * 8));
  ca.tflag = s->tflag.as<int>(); ca.ntri = ntri; ca.qnext = s->flowq.as<int>();
  ca.wsteps = wsteps;
  if (ca.i0)
    launch_init_flow_flags(st, ca.P, ca.tflag, ntri, ntri, (const int*)nullptr, ca.i0);
  else
    HIPCHK(c, hipMemsetAsync(ca.tflag, 0, sizeof(int) * (size_t)ca.P * ntri, st));
  HIPCHK(c, hipMemsetAsync(ca.qnext, 0, sizeof(int) * 8, st));
  launch_flow(dcov, 2 * c->n_cu, st, ca);
  HIPCHK(c, hipGetLastError());
  return AGP_OK;
}

// What the batched sum-of-GPs entries (agp_infer_gp_sum_batch, agp_predict_sum_batch) ask of predict_core on top of pred_code /
// diag_add: each particle's noise_pred on the observable (code 0) query rows only, the dataflow schedule whatever the batch
// (AGP_FLOW=0: the per-column launches) — a particle's bits then do not depend on the batch, its order, copies or chunking — and,
// for predict_sum, the device read-out k_sum_readout: out.mean receives raw means, out.var is not written, out_x [P][m][nq] the
// marginal quantiles, and a particle whose raw marginals fail at row j (0-based) gets info n + j + 1.
struct SumPass {
  bool readout = false;
  int64_t p_rows = 0;                    // query points per component (the F_1 rows)
  double slope = 1.0, intercept = 0.0;
  std::vector<double> z;                 // ndtri(q)
  double* out_x = nullptr;
  int nq() const { return readout ? (int)z.size() : 0; }
};

// What a pass is asked to do on top of the plain joint pass (all optional), and where its results go (per particle of the pass, its
// caller's order).
//   pred_code / diag_add   (per prediction point) what infer_gp_sum adds: component codes of the query points, an extra diagonal term
//   keys                   (per particle) the factor-store keys: a particle whose factor of exactly this prefix is resident (an extension
//                          sweep scored it: the per-step callback of the streaming workload, scripts/online.jl:43, predicts right
//                          after the reweight) skips K11 and its factorisation
//   mix                    (agp_predict_mixture_batch) the chunk's device means and covariances go into the mixture's running sums
//                          (mix_chunk) instead of the outputs: the pass forms every particle's covariance and copies none of them out
struct PassAsk {
  const uint8_t* pred_code = nullptr;
  const double* diag_add = nullptr;
  const std::vector<std::string>* keys = nullptr;
  const SumPass* sum = nullptr;
  MixPass* mix = nullptr;
};
struct PassOut { double* mean = nullptr; double* var = nullptr; double* cov = nullptr; int32_t* info = nullptr; };

// The resident factors a pass starts from (sorted order): store slot per particle, first tile row to compute, and the store's lock
// from the lookup on.
// Resident L^-T: a pass that starts from resident factors AND serves observed points from alpha / diag(K11^-1) keeps Z = L^-T in
// the store beside L (same layout) with the rows' running sums — the next pass on a longer prefix (the per-step callback of a
// stream, scripts/online.jl:43) forms the new tile columns of Z only: nt^2/2 tile products instead of nt^3/6.
// Two invariants, kept by the structure:
//   * the chain kernel advances the slots' running sums on the device; their column counts (zrows) are committed on the host only
//     after the LAST chunk's stream has drained (after_chain).  Any return in between must not leave sums that already include
//     columns the host does not know of: from the first chain launch to the commit the object is armed, and an armed object zeroes
//     the touched entries' zrows when it goes;
//   * that happens under the store's lock: the lock is a member, so the destructor's body runs before the lock is released.
// Lock order: the store's mutex (lookup) before the workspace slot and before c->mu.  The lock goes once the last copy out of the
// store has been made (after_gather), or with resident Z once its new columns are in (after_chain).
struct ResidentFactors {
  agp_ctx* c;
  std::unique_lock<std::mutex> lk;
  int P = 0, n_hit = 0;
  int64_t n = 0;
  std::vector<int32_t> src_slot, i0v, zi0v;
  bool z = false, armed = false;
  const int32_t* d_src = nullptr; const int32_t* d_i0 = nullptr; const int32_t* d_zi0 = nullptr;
  explicit ResidentFactors(agp_ctx* c_) : c(c_) {}
  ~ResidentFactors() { if (armed) for (int32_t sl : src_slot) if (sl >= 0 && (size_t)sl < c->store.zrows.size()) c->store.zrows[(size_t)sl] = 0; }
  ResidentFactors(const ResidentFactors&) = delete; ResidentFactors& operator=(const ResidentFactors&) = delete;

  void lookup(const std::vector<std::string>& keys, const Batch& bt, int P_, const JointPlan& jp) {
    P = P_; n = jp.q.n;
    n_hit = store_lookup(c, keys, bt.order, P, n, jp.nt1, src_slot, i0v, lk);
    std::lock_guard<std::mutex> g(c->mu);
    c->pred_reused += n_hit; c->pred_factored += P - n_hit;
  }
  // the store's Z / zalpha / zdinv (a failed allocation: the pass forms Z in its own scratch), and where each particle's chain starts
  void begin_z() {
    agp_ctx::FactorStore& fs = c->store;
    const size_t before = fs.Z.cap + fs.zalpha.cap + fs.zdinv.cap;
    const size_t rowb = sizeof(double) * (size_t)fs.nt_cap * NB * (size_t)fs.n_slots;
    z = fs.Z.ensure((size_t)fs.strideA * 8 * (size_t)fs.n_slots) == hipSuccess && fs.zalpha.ensure(rowb) == hipSuccess &&
        fs.zdinv.ensure(rowb) == hipSuccess;
    if (!z) { (void)hipGetLastError(); fs.z_release(); }
    const size_t after = fs.Z.cap + fs.zalpha.cap + fs.zdinv.cap;
    fs.footprint = fs.footprint.load() + after - std::min(before, after);
    if (!z) return;
    if (fs.zrows.size() != (size_t)fs.n_slots) fs.zrows.assign((size_t)fs.n_slots, 0);
    // one particle per store entry extends the entry's Z; its copies (a resampled population) work in the sweep's scratch (-1)
    zi0v.assign((size_t)P, 0);
    std::vector<char> taken((size_t)fs.n_slots, 0);
    for (int q = 0; q < P; ++q) {
      const int sl = src_slot[(size_t)q];
      if (sl < 0) continue;
      zi0v[(size_t)q] = taken[(size_t)sl] ? -1 : fs.zrows[(size_t)sl];
      taken[(size_t)sl] = 1;
    }
  }
  int stage(Slot* s, PinnedUploads& up) {
    HIPCHK(c, s->stage.ensure(sizeof(int32_t) * 3 * (size_t)P));
    int32_t* d = s->stage.as<int32_t>();
    up.add(d, src_slot.data(), sizeof(int32_t) * P);
    up.add(d + P, i0v.data(), sizeof(int32_t) * P);
    if (z) { up.add(d + 2 * P, zi0v.data(), sizeof(int32_t) * P); d_zi0 = d + 2 * P; }
    d_src = d; d_i0 = d + P;
    return AGP_OK;
  }
  int after_gather(hipStream_t st, int p_end) {
    if (z || p_end < P) return AGP_OK;
    HIPCHK(c, hipStreamSynchronize(st));
    lk.unlock();
    return AGP_OK;
  }
  void point(GradArgs& ga, int p0) const {
    if (!z) return;
    agp_ctx::FactorStore& fs = c->store;
    ga.lslot = d_src + p0; ga.Lsrc = fs.A.as<double>(); ga.Lstride = fs.strideA; ga.Wsrc = fs.W.as<double>(); ga.Wnt = fs.nt_cap;
    ga.Zsrc = fs.Z.as<double>(); ga.Zstride = fs.strideA; ga.zi0 = d_zi0 + p0;
    ga.zalpha = fs.zalpha.as<double>(); ga.zdinv = fs.zdinv.as<double>(); ga.zld = (long long)fs.nt_cap * NB;
    ga.zfull = (int)(n / NB);
  }
  // Before each chain launch.  NaN-poison mode: what the chain forms again — tile columns >= zi0 of the entry's Z (column i of Z is
  // packed row i) and the running sums of rows >= zi0 (rows below it start from theirs) — reads NaN until written.  Copies (zi0 < 0)
  // are skipped.
  int poison(hipStream_t st, int p0, int Pc) {
    if (!z) return AGP_OK;
    if (c->poison.active()) {
      agp_ctx::FactorStore& fs = c->store;
      PoisonRowsArgs pa = {};
      double* bases[3] = {fs.Z.as<double>(), fs.zalpha.as<double>(), fs.zdinv.as<double>()};
      const long long pitch[3] = {fs.strideA, (long long)fs.nt_cap * NB, (long long)fs.nt_cap * NB};
      const long long unit[3] = {NB2, NB, NB};
      for (int b = 0; b < 3; ++b) { pa.base[b] = bases[b]; pa.pitch[b] = pitch[b]; pa.unit[b] = unit[b]; pa.tri[b] = b == 0; }
      pa.nt_cap = fs.nt_cap; pa.slot = d_src + p0; pa.i0 = d_zi0 + p0;
      launch_poison_rows(st, 256, Pc, 3, pa);
      HIPCHK(c, hipGetLastError());
      for (int q = p0; q < p0 + Pc; ++q) {
        if (src_slot[(size_t)q] < 0 || zi0v[(size_t)q] < 0) continue;
        const long long r0 = std::min<long long>(zi0v[(size_t)q], fs.nt_cap);
        c->poison.count(sizeof(double) * (size_t)((fs.strideA - r0 * (r0 + 1) / 2 * NB2) + 2 * (fs.nt_cap - r0) * NB));
      }
    }
    armed = true;
    return AGP_OK;
  }
  int after_chain(hipStream_t st, int p_end) {
    if (!z || p_end < P) return AGP_OK;
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    // (complete tile columns only: the column of a partly filled last tile is formed again on a longer prefix)
    for (int q = 0; q < P; ++q) if (src_slot[(size_t)q] >= 0) c->store.zrows[(size_t)src_slot[(size_t)q]] = (int32_t)(n / NB);
    armed = false;
    lk.unlock();
    return AGP_OK;
  }
};

int size_buffers(agp_ctx* c, Slot* s, const JointPlan& jp, const SumPass* sum, int P, int chunk) {
  const int64_t m = jp.q.m, m1 = std::max<int64_t>(1, jp.mJ);
  HIPCHK(c, s->A.ensure((size_t)jp.strideA * 8 * chunk));
  if (jp.diag_path) {
    HIPCHK(c, s->Z.ensure((size_t)jp.strideZ * 8 * chunk));
    HIPCHK(c, s->alpha.ensure(sizeof(double) * (size_t)jp.ntot * chunk));
    HIPCHK(c, s->gpart.ensure(sizeof(double) * (size_t)jp.ntot * chunk));      // diag(K11^-1) (the gradient path's scratch, idle here)
  }
  HIPCHK(c, s->W.ensure(sizeof(double) * NSB * 256 * (size_t)chunk * std::max(1, jp.nt1)));     // (the dataflow schedule keeps every column's inverse blocks)
  HIPCHK(c, s->pred_mean.ensure(sizeof(double) * (size_t)m1 * chunk));
  HIPCHK(c, s->pred_var.ensure(sizeof(double) * (size_t)m1 * chunk));
  if (jp.want_cov) HIPCHK(c, s->pred_cov.ensure(sizeof(double) * (size_t)m * m * chunk));
  if (sum && sum->readout) {
    HIPCHK(c, s->sum_x.ensure(sizeof(double) * (size_t)m1 * std::max(1, sum->nq()) * chunk));
    HIPCHK(c, s->sum_z.ensure(sizeof(double) * (size_t)std::max(1, sum->nq())));
    HIPCHK(c, s->out_info.ensure(sizeof(int32_t) * (size_t)P));
  }
  return AGP_OK;
}

// the uploads of the optional modes: codes (padded joint layout), the extra diagonal, the read-out's quantiles, the mixture's weights
int stage_modes(agp_ctx* c, Slot* s, hipStream_t st, PinnedUploads& up, const JointPlan& jp, const PassAsk& ask, const Batch& bt) {
  const int64_t m = jp.q.m, mJ = jp.mJ;
  if (ask.pred_code) {
    std::vector<uint8_t> code((size_t)jp.ntot, 0);
    std::copy(ask.pred_code, ask.pred_code + m, code.begin() + jp.n1_pad);
    HIPCHK(c, s->code.ensure((size_t)jp.ntot));
    up.add(s->code.p, code.data(), (size_t)jp.ntot);
  }
  if (ask.diag_add && mJ > 0) {
    HIPCHK(c, s->diag_add.ensure(sizeof(double) * (size_t)mJ));
    up.add(s->diag_add.p, jp.daddJ, sizeof(double) * mJ);
  }
  if (ask.sum && ask.sum->nq() > 0) up.add(s->sum_z.p, ask.sum->z.data(), sizeof(double) * ask.sum->nq());
  if (ask.mix) {
    std::vector<double> w_pass(bt.order.size());
    for (size_t q = 0; q < w_pass.size(); ++q) w_pass[q] = ask.mix->w[(size_t)bt.order[q]];
    if (const int rc = mix_stage(c, s, st, up, *ask.mix, m, w_pass)) return rc;
  }
  return AGP_OK;
}

// The slot's pinned landing zone for sorted positions [p0, p0 + Pc): [mean | var | alpha | dinv | x], the middle two on the
// training-point route only, x [Pc][mJ][nq].
struct Landing { int p0, Pc; double* mean; double* var; double* alpha; double* dinv; double* x; };
int landing_zone(agp_ctx* c, Slot* s, const JointPlan& jp, int nq, int p0, int Pc, Landing& h) {
  const size_t nm = (size_t)std::max<int64_t>(1, jp.mJ) * Pc, nd = jp.diag_path ? (size_t)jp.ntot * Pc : 0;
  HIPCHK(c, s->h_out.ensure(sizeof(double) * (2 * nm + 2 * nd + nm * nq)));
  double* hz = static_cast<double*>(s->h_out.p);
  h = {p0, Pc, hz, hz + nm, hz + 2 * nm, hz + 2 * nm + nd, hz + 2 * nm + 2 * nd};
  return AGP_OK;
}

// Z = L11^-T row chains; alpha = Z beta and diag(K11^-1) = row sums of Z.^2 come out of the same registers
int z_chain(agp_ctx* c, Slot* s, hipStream_t st, const JointPlan& jp, ResidentFactors& rf, const Landing& h) {
  const int Pc = h.Pc, ntot = jp.ntot;
  GradArgs ga = {};
  ga.A = s->A.as<double>(); ga.strideA = jp.strideA; ga.Z = s->Z.as<double>(); ga.strideZ = jp.strideZ; ga.W = s->W.as<double>();
  ga.beta = s->vec.as<double>(); ga.alpha = s->alpha.as<double>(); ga.dinv = s->gpart.as<double>(); ga.ldv = ntot;
  ga.P = Pc; ga.nt = jp.nt1; ga.n = (int)jp.q.n;
  rf.point(ga, h.p0);
  if (const int rc = rf.poison(st, h.p0, Pc)) return rc;
  launch_trtri_chain(st, 8 * ((Pc + 7) / 8) * jp.nt1, ga);
  if (const int rc = rf.after_chain(st, h.p0 + Pc)) return rc;
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(h.alpha, s->alpha.p, sizeof(double) * ntot * Pc, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(h.dinv, s->gpart.p, sizeof(double) * ntot * Pc, hipMemcpyDeviceToHost, st));
  return AGP_OK;
}

// Schur complement of the prediction block + (-V^T alpha); with nt1 == 0 this just passes K22 through.  Without a covariance request
// only the diagonal tiles are updated: mean and marginal variances cost n^3/3 + n^2 m instead of n^3/3 + n^2 m + n m^2.
int launch_schur(agp_ctx* c, hipStream_t st, const JointPlan& jp, const Batch& bt, JointChunk& k) {
  CholArgs& ca = k.ca;
  ca.schur_diag_only = jp.want_cov ? 0 : 1;
  const int T = jp.want_cov ? jp.nt2 * (jp.nt2 + 1) / 2 : jp.nt2;
  const int Pg = (ca.P + 7) / 8;
  int dcov_s = k.dcov;
  if (jp.lagr() && k.nf > 0) {
    // (the Schur kernel has no table-reading instantiation: the prediction block's tiles of the particles that evaluated
    // their other tiles in-kernel come from k_cov_tiles, which reads the rank tables in place)
    CovArgs cp = k.cv;
    cp.p_off = 0; cp.pred_only = 1; cp.i0 = nullptr;
    HIPCHK(c, launch_cov(st, cp, jp.ntiles, k.nf, bt.max_cp, bt.max_depth, bt.max_ops));
    ca.n_fused = 0; dcov_s = 0;
  }
  launch_update_schur(dcov_s, 8 * Pg * T, st, ca);
  return AGP_OK;
}

// means, variances (covariances) of the chunk's joint query points out of the Schur complement: s->pred_mean / pred_var / pred_cov
int extract_chunk(agp_ctx* c, Slot* s, hipStream_t st, const JointPlan& jp, const PassAsk& ask, int p0, int Pc) {
  PredArgs pa = {};
  pa.A = s->A.as<double>(); pa.strideA = jp.strideA; pa.vec = s->vec.as<double>(); pa.ldv = jp.ntot;
  pa.mu2 = jp.q.mean_pred ? s->mu2.as<double>() : nullptr; pa.noise_pred = s->noise_pred.as<double>() + p0;
  pa.nt1 = jp.nt1; pa.n1_pad = jp.n1_pad; pa.m = (int)jp.mJ; pa.P = Pc;
  pa.diag_add = ask.diag_add ? s->diag_add.as<double>() : nullptr;
  pa.np_code = ask.sum ? s->code.as<uint8_t>() + jp.n1_pad : nullptr;
  pa.out_mean = s->pred_mean.as<double>(); pa.out_var = s->pred_var.as<double>();
  pa.out_cov = jp.want_cov ? s->pred_cov.as<double>() : nullptr;
  const long long nel = jp.want_cov ? (long long)jp.mJ * jp.mJ : (long long)jp.mJ;
  launch_pred_extract(st, nel, Pc, pa);
  HIPCHK(c, hipGetLastError());
  return AGP_OK;
}

// predict_sum's device read-out of the chunk (k_sum_readout) and its quantiles on their way to the landing zone
int sum_readout_chunk(agp_ctx* c, Slot* s, hipStream_t st, const JointPlan& jp, const SumPass& sum, const Landing& h) {
  const int nq = sum.nq();
  SumReadArgs ra = {};
  ra.mean = s->pred_mean.as<double>(); ra.var = s->pred_var.as<double>(); ra.m = (int)jp.mJ; ra.p_rows = (int)sum.p_rows;
  ra.slope = sum.slope; ra.intercept = sum.intercept; ra.shift = sum.intercept / sum.slope;
  ra.ivar = 1.0 / (sum.slope * sum.slope);
  ra.z = s->sum_z.as<double>(); ra.nq = nq; ra.x = s->sum_x.as<double>(); ra.bad = s->out_info.as<int32_t>() + h.p0;
  launch_sum_readout(st, h.Pc, ra);
  HIPCHK(c, hipGetLastError());
  if (nq > 0) HIPCHK(c, hipMemcpyAsync(h.x, s->sum_x.p, sizeof(double) * jp.mJ * nq * h.Pc, hipMemcpyDeviceToHost, st));
  return AGP_OK;
}

// The landed chunk (sorted order) to the caller's particle order.  Training-point route: the joint results go to their query
// positions fq, the training-time queries are recombined on the host,
//     mean = mu2 + (y - mu1) - noise alpha,      var = noise - noise^2 dinv + noise_pred (+ diag_add).
void scatter_chunk(agp_ctx* c, const JointPlan& jp, const PassAsk& ask, const PassOut& out, const Batch& bt, const SortedNoise& nz,
                   const Landing& h) {
  const int64_t m = jp.q.m, mJ = jp.mJ;
  const double* mean_train = jp.q.mean_train; const double* mean_pred = jp.q.mean_pred;
  const bool ro = ask.sum && ask.sum->readout;
  const int nq = ask.sum ? ask.sum->nq() : 0;
  for (int q = 0; q < h.Pc; ++q) {
    const size_t o = (size_t)bt.order[h.p0 + q];
    if (jp.diag_path) {
      double* om = out.mean + o * m; double* ov = out.var + o * m;
      for (int64_t g = 0; g < mJ; ++g) { om[jp.fq[(size_t)g]] = h.mean[(size_t)q * mJ + g]; ov[jp.fq[(size_t)g]] = h.var[(size_t)q * mJ + g]; }
      const double s2 = nz.noise[(size_t)h.p0 + q], np2 = nz.pred[(size_t)h.p0 + q];
      const double* al = h.alpha + (size_t)q * jp.ntot; const double* dv = h.dinv + (size_t)q * jp.ntot;
      for (size_t d = 0; d < jp.dq.size(); ++d) {
        const int32_t j = jp.dq[d], i = jp.di[d];
        const double ymu = c->h_xs[(size_t)i] - (mean_train ? mean_train[i] : 0.0);
        om[j] = (mean_pred ? mean_pred[j] : 0.0) + ymu - s2 * al[i];
        ov[j] = s2 - s2 * s2 * dv[i] + np2 + (ask.diag_add ? ask.diag_add[j] : 0.0);
      }
      continue;
    }
    std::memcpy(out.mean + o * m, h.mean + (size_t)q * m, sizeof(double) * m);
    if (!ro) std::memcpy(out.var + o * m, h.var + (size_t)q * m, sizeof(double) * m);
    if (nq > 0) std::memcpy(ask.sum->out_x + o * m * nq, h.x + (size_t)q * m * nq, sizeof(double) * m * nq);
  }
}

// The info pass after the last chunk.  Always made: a caller that passes out.info = NULL must still never receive unmarked garbage.
int finish_info(agp_ctx* c, Slot* s, hipStream_t st, const JointPlan& jp, const PassAsk& ask, const PassOut& out, const Batch& bt) {
  const int64_t n = jp.q.n, m = jp.q.m;
  const int P = (int)bt.order.size();
  const bool ro = ask.sum && ask.sum->readout;
  const int nq = ask.sum ? ask.sum->nq() : 0;
  std::vector<int32_t> info_sorted(P), bad_sorted(ro ? P : 0);
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipMemcpy(info_sorted.data(), s->info.p, sizeof(int32_t) * P, hipMemcpyDeviceToHost));      // (blocking: nothing in flight towards the local on an error return)
  if (ro) HIPCHK(c, hipMemcpy(bad_sorted.data(), s->out_info.p, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
  for (int q = 0; q < P; ++q) {
    if (info_sorted[q] < 0) return fail(c, AGP_ERR_HIP, "in-kernel panel solve timed out waiting for its diagonal factor");
    const int p = bt.order[q];
    // (predict_sum: a factor that failed comes first; then the first row of raw marginals that fails)
    if (ro && info_sorted[q] == 0 && bad_sorted[q] >= 1 && bad_sorted[q] <= m) info_sorted[q] = (int32_t)(n + bad_sorted[q]);
    if (out.info) out.info[p] = info_sorted[q];
    if (info_sorted[q] != 0) {
      const double nanv = std::nan("");
      for (int64_t g = 0; g < m && out.mean; ++g) { out.mean[(size_t)p * m + g] = nanv; if (out.var) out.var[(size_t)p * m + g] = nanv; }
      if (out.cov) for (int64_t g = 0; g < m * m; ++g) out.cov[(size_t)p * m * m + g] = nanv;
      if (nq > 0) std::fill(ask.sum->out_x + (size_t)p * m * nq, ask.sum->out_x + (size_t)(p + 1) * m * nq, nanv);
    }
  }
  return AGP_OK;
}

// Core of the predictive path (src/GP.jl:739-757) for a compiled batch (bt: pp's programs, compiled) over the plan `jp` its entry made.
int predict_core(agp_ctx* c, const Particles& pp, Batch& bt, const JointPlan& jp, const PassAsk& ask, const PassOut& out) {
  const int64_t n = jp.q.n, m = jp.q.m, mJ = jp.mJ;
  const int P = pp.P;
  const int nt1 = jp.nt1, ntot = jp.ntot;
  const SumPass* sum = ask.sum; MixPass* mix = ask.mix;
  const bool ro = sum && sum->readout;
  const int nq = sum ? sum->nq() : 0;
  if (jp.want_cov != (out.cov != nullptr || (mix && mix->cov)) || jp.has_codes != (ask.pred_code != nullptr) || (int)bt.order.size() != P)
    return fail(c, AGP_ERR_ARG, "the joint plan was made for another pass");
  // ---- store lookup (the store's lock before the slot) ----
  ResidentFactors rf(c);
  if (ask.keys && c->predict_reuse && nt1 > 0 && !jp.q.mean_train && !ask.pred_code) rf.lookup(*ask.keys, bt, P, jp);
  const int n_hit = rf.n_hit;
  // ---- slot and stream ----
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  // ---- buffer sizes, uploads, one flush ----
  const int chunk = jp.chunk(c, P);
  if (const int rc = size_buffers(c, s, jp, sum, P, chunk)) return rc;
  PinnedUploads up;
  SortedNoise nz;
  if (const int rc = stage_joint(c, s, up, jp, pp, bt, chunk, nz)) return rc;
  if (const int rc = stage_modes(c, s, st, up, jp, ask, bt)) return rc;
  if (n_hit > 0 && jp.diag_path) rf.begin_z();
  if (n_hit > 0)
    if (const int rc = rf.stage(s, up)) return rc;
  if (const int rc = flush_uploads(c, s, st, up, bt, jp)) return rc;

  if (ro) HIPCHK(c, hipMemsetAsync(s->out_info.p, 0x7f, sizeof(int32_t) * (size_t)P, st));      // (no failing row: 0x7f7f7f7f)
  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int Pc = std::min(chunk, P - p0);
    Landing h;
    if (const int rc = landing_zone(c, s, jp, nq, p0, Pc, h)) return rc;
    // ---- init, gather ----
    launch_init_vec(st, ntot, Pc, s->vec.as<double>(), c->d_xs, (jp.q.mean_train && n > 0) ? s->mu1.as<double>() : (const double*)nullptr, (int)n, s->info.as<int>() + p0, s->ready.as<int>() + p0);
    if (n_hit > 0) {
      launch_gather(c, st, Pc, nt1, s->A.as<double>(), jp.strideA, s->W.as<double>(), nt1, s->vec.as<double>(), ntot, nullptr, 0,
                    rf.d_src + p0, s->ready.as<int>() + p0);
      HIPCHK(c, hipGetLastError());
      // (Reading L11 and the inverse blocks in place — a second base pointer for the training rows in chol_tile — was
      // measured: the streamed config 5 went 412 -> 406 ms, the dataflow kernel gained 4 spilled VGPRs; the copy stays.)
      if (const int rc = rf.after_gather(st, p0 + Pc)) return rc;
    }
    // ---- tiles ----
    JointChunk k = chunk_setup(s, jp, bt, p0, Pc);
    CholArgs& ca = k.ca;
    k.cv.code = ca.code = ask.pred_code ? s->code.as<uint8_t>() : nullptr;
    k.cv.skip_pred_offdiag = jp.want_cov ? 0 : 1;
    k.cv.i0 = ca.i0 = n_hit > 0 ? rf.d_i0 + p0 : nullptr;
    if (n_hit > 0 || jp.diag_path) ca.wsteps = nt1;      // panel solves of the prediction rows / the chains of Z read every column's inverse blocks
    HIPCHK(c, launch_cov(st, k.cv, jp.ntiles, Pc - k.nf, bt.max_cp, bt.max_depth, bt.max_ops));
    // ---- factor ----
    if (nt1 > 0 && (sum ? c->flow != 0 : use_flow(c, Pc, jp.nt, nt1))) {
      // dataflow schedule over the block columns of the training block (all rows: V = L^-1 K12 comes out of the same tiles)
      if (const int rc = launch_joint_flow(c, s, st, ca, k.dcov, nt1)) return rc;
    } else if (n_hit > 0) {
      // (invariant of every branch here: only the training block's nt1 columns are factored, so the diagonal-tile kernel sees
      // tiles with n1 - tk * NB > 0 rows of data; the query rows below them are panel solves, never a diagonal step)
      // per-column launches restricted to the rows some particle still has to compute
      int i0min = nt1;
      for (int q = 0; q < Pc; ++q) i0min = std::min(i0min, (int)rf.i0v[(size_t)p0 + q]);
      HIPCHK(c, run_factor_extend(st, ca, k.dcov, use_split_diag(c, ca.P), i0min, nt1));
    } else {
      HIPCHK(c, run_factor(st, ca, nt1, k.dcov, nullptr, nullptr, use_split_diag(c, ca.P)));
    }
    // ---- Z chain, Schur, extract, mode read-outs, copy-back ----
    if (jp.diag_path)
      if (const int rc = z_chain(c, s, st, jp, rf, h)) return rc;
    if (mJ > 0) {
      if (const int rc = launch_schur(c, st, jp, bt, k)) return rc;
      if (const int rc = extract_chunk(c, s, st, jp, ask, p0, Pc)) return rc;
      if (mix)      // (before the next chunk overwrites pred_mean / pred_cov)
        if (const int rc = mix_chunk(c, s, st, *mix, p0, Pc, s->pred_mean.as<double>(), s->pred_var.as<double>(),
                                     jp.want_cov ? s->pred_cov.as<double>() : nullptr)) return rc;
      if (ro)
        if (const int rc = sum_readout_chunk(c, s, st, jp, *sum, h)) return rc;
      // results come back in sorted order (a mixture pass returns no per-particle marginals)
      if (!mix) HIPCHK(c, hipMemcpyAsync(h.mean, s->pred_mean.p, sizeof(double) * mJ * Pc, hipMemcpyDeviceToHost, st));
      if (!ro && !mix) HIPCHK(c, hipMemcpyAsync(h.var, s->pred_var.p, sizeof(double) * mJ * Pc, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipStreamSynchronize(st));
    if (!mix) scatter_chunk(c, jp, ask, out, bt, nz, h);
    for (int q = 0; q < Pc && out.cov && !mix; ++q)
      HIPCHK(c, hipMemcpyAsync(out.cov + (size_t)bt.order[p0 + q] * m * m, s->pred_cov.as<double>() + (size_t)q * m * m,
                               sizeof(double) * m * m, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
  }
  if (mix)
    if (const int rc = mix_finish(c, s, st, *mix)) return rc;
  return finish_info(c, s, st, jp, ask, out, bt);
}

// Predictive log-density (src/api.jl:686-699, test/experiment_hmc.jl:125): logpdf(MvNormal(node, noise, ts[1:n], xs[1:n], ts_pred;
// noise_pred, mean), y_pred) for a compiled batch.  predict_core's joint matrix [K11 + noise I, K12; K21, K22 + noise_pred I] is
// factored through ALL nt1 + nt2 block columns with [x - mu1; y_pred - mu2] in the forward solve: the query block of the factor is
// the Cholesky factor of Sigma* = K22 - K21 K11^-1 K12 + noise_pred I and its forward solve L22^-1 (y* - mu*), so the query columns'
// partials are log|Sigma*| and the Mahalanobis term themselves (k_finish_pred_logpdf) — no Schur step, no read-out, and no
// difference of two large log-likelihoods.  (No duplicate-query shortcut: it yields diag(Sigma*), not Sigma* — its plan is made with
// want_cov.)  y_pred == nullptr (agp_predict_sample_batch): the query part of the right-hand side is 0.  `hooks` (nullable): see
// JointHooks.
int predict_logpdf_core(agp_ctx* c, const JointPlan& jp, const double* y_pred, const Particles& pp, Batch& bt, double* out_lp,
                        int32_t* out_info, JointHooks* hooks) {
  const int64_t n = jp.q.n, m = jp.q.m;
  const int P = pp.P;
  const int nt1 = jp.nt1, nt = jp.nt, ntot = jp.ntot;
  const int chunk = jp.chunk(c, P);

  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;

  HIPCHK(c, s->A.ensure((size_t)jp.strideA * 8 * chunk));
  HIPCHK(c, s->W.ensure(sizeof(double) * NSB * 256 * (size_t)chunk * nt));     // (the dataflow schedule keeps every column's inverse blocks)
  HIPCHK(c, s->pred_mean.ensure(sizeof(double) * (size_t)m));      // y_pred (the read-out buffers are idle in this pass)
  HIPCHK(c, s->map.ensure(sizeof(int32_t) * (size_t)P));
  HIPCHK(c, s->out_lp.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->out_info.ensure(sizeof(int32_t) * (size_t)P));
  PinnedUploads up;
  SortedNoise nz;
  if (const int rc = stage_joint(c, s, up, jp, pp, bt, chunk, nz)) return rc;
  if (y_pred) up.add(s->pred_mean.p, y_pred, sizeof(double) * m);
  up.add(s->map.p, bt.order.data(), sizeof(int32_t) * P);
  if (hooks && hooks->stage)
    if (const int rc = hooks->stage(s, up, chunk)) return rc;
  if (const int rc = flush_uploads(c, s, st, up, bt, jp)) return rc;

  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int Pc = std::min(chunk, P - p0);
    launch_init_vec(st, ntot, Pc, s->vec.as<double>(), c->d_xs, (jp.q.mean_train && n > 0) ? s->mu1.as<double>() : (const double*)nullptr,
                    (int)n, s->info.as<int>() + p0, s->ready.as<int>() + p0);
    if (y_pred)
      launch_init_query_vec(st, Pc, s->vec.as<double>(), ntot, jp.n1_pad, (int)m, s->pred_mean.as<double>(),
                            jp.q.mean_pred ? s->mu2.as<double>() : (const double*)nullptr);
    JointChunk k = chunk_setup(s, jp, bt, p0, Pc);
    CholArgs& ca = k.ca;
    k.cv.noise_q = ca.noise_q = s->noise_pred.as<double>() + p0;
    ca.nt1 = nt;      // (every block column is factored)
    HIPCHK(c, launch_cov(st, k.cv, jp.ntiles, Pc - k.nf, bt.max_cp, bt.max_depth, bt.max_ops));
    // (one schedule whatever the batch: a particle's log-density does not depend on the particles around it — the per-column
    // launches only where the dataflow schedule is switched off, AGP_FLOW=0)
    if (c->flow != 0) {
      if (const int rc = launch_joint_flow(c, s, st, ca, k.dcov, nt)) return rc;
    } else {
      HIPCHK(c, run_factor(st, ca, nt, k.dcov, nullptr, nullptr, use_split_diag(c, ca.P)));
    }
    launch_finish_pred_logpdf(st, ca.partial, ca.info, nt1, nt, Pc, (int)m, (int)n, jp.n1_pad, s->map.as<int32_t>() + p0,
                              s->out_lp.as<double>(), s->out_info.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    if (hooks && hooks->chunk)      // (before the next chunk overwrites A)
      if (const int rc = hooks->chunk(s, st, ca, p0, Pc)) return rc;
  }
  // (results are in the caller's order already; blocking copies: nothing in flight towards the locals on an error return)
  std::vector<int32_t> info(P);
  HIPCHK(c, hipStreamSynchronize(st));
  HIPCHK(c, hipMemcpy(out_lp, s->out_lp.p, sizeof(double) * P, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(info.data(), s->out_info.p, sizeof(int32_t) * P, hipMemcpyDeviceToHost));
  for (int p = 0; p < P; ++p) {
    if (info[p] < 0) return fail(c, AGP_ERR_HIP, "in-kernel panel solve timed out waiting for its diagonal factor");
    if (out_info) out_info[p] = info[p];
  }
  if (hooks && hooks->done)
    if (const int rc = hooks->done(s)) return rc;
  return AGP_OK;
}

}  // namespace

namespace {

// Structured predictive pass (no dense factor) for the Toeplitz + rank-2 class: training points = n consecutive grid points, query
// points = any of them and/or grid points that follow them.  One Schur recursion over the JOINT grid (n + m_f points) leaves, per
// future point, L21 L11^-1 [x, 1, t] and the diagonal of T22 - T21 T11^-1 T12 (k_toep_logpdf<.., JOINT>); the backward substitution
// over the training block gives T11^-1 [x, e_first, 1, t].  The rest is O(n + m) per particle on the host:
//   K11^-1 x = alpha = a - W S U'a,   (K11^-1)_uu = (T11^-1)_uu - w_u' S w_u,   (T11^-1)_uu = sum_{i<=u} (x_i^2 - y_i^2) / x_0  (Gohberg-Semencul),
//   future point f:  mean = m_x + r' S U'a  (= m_x - m_U' S U'a + h_f' C U'alpha, since C (I - N S) = S),   var = s_f - noise + r' S r + noise_pred,  r = h_f - m_U
// (a Gaussian process plus a Bayesian linear model in the basis [1, t]: Rasmussen & Williams (2.42)), S = C (I + N C)^-1, N = U'W;
// training point u:  mean = x_u - noise alpha_u,  var = noise - noise^2 (K11^-1)_uu + noise_pred  (x: the residual x - mean_train; mean_pred is added to every prediction).
// qkind[j] >= 0: query j is training point with sorted position qkind[j];  < 0: future point -1 - qkind[j].
int toeplitz_predict_sweep(agp_ctx* c, const PredQuery& q, const Particles& pp, int32_t rank0, int mF, const PredLattice& pl,
                           const std::vector<int32_t>& qkind, const std::vector<double>& xq, double* out_mean, double* out_var,
                           int32_t* out_info, const double* xs_sorted_host) {
  // xs_sorted_host (nullable): x - mean_train at the n training points in sorted order (mean functions: the recursion then runs on
  // the residuals; xq holds the same residuals for the observed query points); q.mean_pred (nullable, per query) is added at the end
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t n = q.n, m = q.m;
  const int P = pp.P;
  const double* noise = pp.noise; const double* noise_pred = pp.noise_pred; const double* mean_pred = q.mean_pred;
  Batch bt;
  CompileOpts co;
  co.lag = true; co.lag_units = pl.rank_units; co.rank_extra = 1;
  int rc = compile_batch(c, pp, bt, co);
  if (rc) return rc;
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const int n_pad = round_up(n, NB), mF_pad = std::max(NB, round_up(mF, NB));
  const int N = (int)n + mF;
  std::vector<double> nz((size_t)P);
  for (int q = 0; q < P; ++q) nz[(size_t)q] = noise[bt.order[q]];
  const long long Lstride = (long long)n * (n + 1) / 2;
  const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(P, ws_limit_bytes(c) / (Lstride * 8)));
  const int stride = pl.rank_units * 256;
  HIPCHK(c, s->hdr.ensure(sizeof(ProgHdr) * (size_t)P));
  HIPCHK(c, s->ops.ensure(bt.ops.size() + 4));
  HIPCHK(c, s->prm.ensure(sizeof(double) * std::max<size_t>(1, bt.prm.size())));
  HIPCHK(c, s->noise.ensure(sizeof(double) * (size_t)P));
  HIPCHK(c, s->pl_tl.ensure(sizeof(double) * pl.tl.size()));
  HIPCHK(c, s->out_lp.ensure(sizeof(double) * (size_t)P + sizeof(int32_t) * (size_t)P));
  HIPCHK(c, s->A.ensure((size_t)Lstride * 8 * chunk));
  HIPCHK(c, s->tsol.ensure(sizeof(double) * 4 * (size_t)n_pad * chunk));
  HIPCHK(c, s->alpha.ensure(sizeof(double) * 4 * (size_t)n_pad * chunk));
  HIPCHK(c, s->pred_mean.ensure(sizeof(double) * 4 * (size_t)mF_pad * chunk));
  HIPCHK(c, s->lagtab.ensure(sizeof(double) * std::max<size_t>(16, (size_t)bt.n_lag_tables * stride)));
  PinnedUploads up;
  up.add(s->hdr.p, bt.hdr.data(), sizeof(ProgHdr) * (size_t)P);
  up.add(s->ops.p, bt.ops.data(), bt.ops.size());
  up.add(s->prm.p, bt.prm.data(), sizeof(double) * bt.prm.size());
  up.add(s->noise.p, nz.data(), sizeof(double) * (size_t)P);
  const LagProgLayout lpl(bt);
  HIPCHK(c, lpl.upload(up, s->pl_prog));
  up.add(s->pl_tl.p, pl.tl.data(), sizeof(double) * pl.tl.size());
  if (xs_sorted_host) {
    HIPCHK(c, s->mu1.ensure(sizeof(double) * (size_t)n));
    up.add(s->mu1.p, xs_sorted_host, sizeof(double) * (size_t)n);
  }
  HIPCHK(c, up.flush(s->h_stage, s->up_blob, st));
  if (bt.n_lag_tables > 0) {
    LagArgs la = {};
    la.tt = s->pl_tl.as<double>(); la.tab = s->lagtab.as<double>();
    lpl.point(la, s->pl_prog.p);
    la.nt = 2 * pl.rank_units; la.full = 1; la.stride = stride;
    launch_lag_tables(st, la, pl.rank_units, bt.n_lag_tables);
    HIPCHK(c, hipGetLastError());
  }
  const double h = c->grid_h;
  auto tau_of = [&](int u) { return ((double)(rank0 + u) - c->grid_mid) * h; };
  std::vector<double> Tdiag((size_t)n), alpha((size_t)n);
  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int Pc = std::min(chunk, P - p0);
    ToepArgs ta = {};
    ta.xs = xs_sorted_host ? s->mu1.as<double>() : c->d_xs_s + rank0; ta.n = (int)n; ta.nj = N; ta.P = Pc; ta.rank0 = rank0;
    ta.hdr = s->hdr.as<ProgHdr>() + p0; ta.ops = s->ops.as<uint8_t>(); ta.prm = s->prm.as<double>(); ta.noise = s->noise.as<double>() + p0;
    ta.lagtab = s->lagtab.as<double>(); ta.lag_stride = stride;
    ta.grid_h = h; ta.grid_mid = c->grid_mid; ta.tref = c->t_ref;
    ta.out_lp = s->out_lp.as<double>() + p0; ta.out_info = reinterpret_cast<int32_t*>(s->out_lp.as<double>() + P) + p0;
    ta.Lcols = s->A.as<double>(); ta.Lstride = Lstride; ta.fwd = s->alpha.as<double>(); ta.sol = s->tsol.as<double>(); ta.ldv = n_pad;
    ta.pacc = s->pred_mean.as<double>(); ta.pstride = mF_pad;
    HIPCHK(c, launch_toep_logpdf(st, ta));
    const size_t nsol = (size_t)4 * n_pad * Pc, nacc = (size_t)4 * mF_pad * Pc;
    HIPCHK(c, s->h_out.ensure(sizeof(double) * (nsol + nacc) + sizeof(int32_t) * (size_t)Pc));
    double* hs = static_cast<double*>(s->h_out.p);
    double* ha = hs + nsol;
    int32_t* hi = reinterpret_cast<int32_t*>(ha + nacc);
    HIPCHK(c, hipMemcpyAsync(hs, s->tsol.p, sizeof(double) * nsol, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ha, s->pred_mean.p, sizeof(double) * nacc, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(hi, ta.out_info, sizeof(int32_t) * (size_t)Pc, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int q = 0; q < Pc; ++q) {
      const int pc = bt.order[p0 + q];
      out_info[pc] = hi[q];
      double* om = out_mean + (size_t)pc * m; double* ov = out_var + (size_t)pc * m;
      if (hi[q] != 0) continue;
      const double s2 = noise[pc], s2p = noise_pred ? noise_pred[pc] : noise[pc];
      const double* a_ = hs + (size_t)q * 4 * n_pad; const double* x_ = a_ + n_pad; const double* w1 = x_ + n_pad; const double* wt = w1 + n_pad;
      const double* mx = ha + (size_t)q * 4 * mF_pad; const double* m1 = mx + mF_pad; const double* mt = m1 + mF_pad; const double* sT = mt + mF_pad;
      // C: the Linear leaves (device form: intercept, bias, amplitude) in the basis [1, t - t_ref]
      double C00 = 0.0, C01 = 0.0, C11 = 0.0;
      {
        const ProgHdr& ph = bt.hdr[p0 + q];
        int qi = 0;
        for (int ip = 0; ip < ph.n_ops; ++ip) {
          const int o = bt.ops[(size_t)ph.op_off + ip];
          if (o == OP_LIN) {
            const double* pr = bt.prm.data() + ph.prm_off + qi;
            const double cc = pr[0] - c->t_ref;
            C00 += pr[1] + pr[2] * cc * cc; C01 -= pr[2] * cc; C11 += pr[2];
          }
          qi += (o == OP_WN || o == OP_CONST) ? 1 : (o == OP_LIN) ? 3 : 0;
        }
      }
      double N00 = 0.0, N01 = 0.0, N11 = 0.0, ux0 = 0.0, ux1 = 0.0;
      const bool lin = C00 != 0.0 || C01 != 0.0 || C11 != 0.0;
      if (lin)
        for (int u = 0; u < n; ++u) { const double t = tau_of(u); N00 += w1[u]; N01 += wt[u]; N11 += t * wt[u]; ux0 += a_[u]; ux1 += t * a_[u]; }
      const double t00 = 1.0 + (N00 * C00 + N01 * C01), t01 = N00 * C01 + N01 * C11, t10 = N01 * C00 + N11 * C01, t11 = 1.0 + (N01 * C01 + N11 * C11);
      const double idet = 1.0 / (t00 * t11 - t01 * t10);
      const double i00 = t11 * idet, i01 = -t01 * idet, i10 = -t10 * idet, i11 = t00 * idet;
      const double S00 = C00 * i00 + C01 * i10, S01 = C00 * i01 + C01 * i11, S11 = C01 * i01 + C11 * i11;
      const double as0 = S00 * ux0 + S01 * ux1, as1 = S01 * ux0 + S11 * ux1;
      // diag(T11^-1) by Gohberg-Semencul (cumulative), alpha
      {
        const double ix0 = 1.0 / x_[0];
        double cum = 0.0;
        for (int u = 0; u < n; ++u) {
          const double xu = x_[u], yu = u == 0 ? 0.0 : x_[n - u];
          cum += (xu - yu) * (xu + yu);
          Tdiag[(size_t)u] = cum * ix0;
          alpha[(size_t)u] = lin ? a_[u] - (w1[u] * as0 + wt[u] * as1) : a_[u];
        }
      }
      for (int64_t j = 0; j < m; ++j) {
        const int kq = qkind[(size_t)j];
        if (kq >= 0) {
          const int u = kq;
          const double kd = lin ? Tdiag[(size_t)u] - (w1[u] * (S00 * w1[u] + S01 * wt[u]) + wt[u] * (S01 * w1[u] + S11 * wt[u])) : Tdiag[(size_t)u];
          om[j] = xq[(size_t)j] - s2 * alpha[(size_t)u];
          ov[j] = s2 - s2 * s2 * kd + s2p;
        } else {
          const int f = -1 - kq;
          double mean = mx[f], var = sT[f] - s2;
          if (lin) {
            const double tf = tau_of((int)n + f);
            const double r0_ = 1.0 - m1[f], r1_ = tf - mt[f];
            mean += r0_ * as0 + r1_ * as1;     // h_f' C U'alpha = h_f' S U'a exactly (C (I - N S) = S): no difference of near-equal terms
            var += r0_ * (S00 * r0_ + S01 * r1_) + r1_ * (S01 * r0_ + S11 * r1_);
          }
          om[j] = mean; ov[j] = var + s2p;
        }
        if (mean_pred) om[j] += mean_pred[j];
      }
    }
  }
  return AGP_OK;
}

thread_local bool tl_in_tpredict = false;

// The dense pass of agp_predict_batch.  `mix` (nullable, with the caller particles' `weights`; agp_predict_mixture_batch's covariance
// pass): the same pass with a covariance request, the per-particle covariances reduced on the device (predict_core's MixPass) and no
// per-particle output but out_info.
int predict_dense(agp_ctx* c, const PredQuery& q, const Particles& pp, double* out_mean, double* out_var, double* out_cov, int32_t* out_info,
                  const double* weights, MixPass* mix) {
  const int64_t n = q.n, m = q.m;
  const bool want_cov = out_cov != nullptr || (mix && mix->cov);
  // A resampled population holds copies of the survivors (src/inference_smc_anneal_data.jl:198-204) and the reference
  // predicts particle by particle (src/api.jl:508-520): each distinct (program, parameters, noise, noise_pred) runs once.
  const Distinct D(pp, c->dedup != 0);      // (malformed offsets: no dedup)
  const Particles run = D.run();
  const int U = D.U();
  if (mix) {
    // (copies: their weights are added, in the caller's order, onto the representative)
    mix->w.assign((size_t)U, 0.0);
    for (int p = 0; p < pp.P; ++p) mix->w[(size_t)D.rep_of(p)] += weights[p];
    std::lock_guard<std::mutex> g(c->mu);
    c->n_particles_seen += pp.P; c->n_particles_run += U;      // (agp_get_dedup_stats)
  }
  // (a store that holds nothing is not consulted: no key strings are built)
  const bool want_keys = c->predict_reuse && n > 0 && !q.mean_train && c->store.n_slots > 0;
  PredLattice pl;
  predict_lattice(c, n, q.ts_pred, m, pl);
  JointPlan jp;              // (before the batch is compiled: the schedule hints see the joint matrix that will run)
  plan_joint(c, q, want_cov, false, nullptr, &pl, jp);
  Batch bt;
  CompileOpts co;
  co.fuse_hint = co.flow_limit = n > 0 && use_flow(c, U, jp.nt, jp.nt1);
  co.lag = pl.on; co.lag_units = pl.on ? pl.rank_units : 1; co.rank_extra = pl.on;
  int rc = compile_batch(c, run, bt, co);
  if (rc) return rc;
  std::vector<std::string> keys;
  if (want_keys)
    for (int u = 0; u < U; ++u) keys.push_back(particle_key(run, u));
  auto core = [&](double* om, double* ov, double* oc, int32_t* oi) {
    PassAsk ask; ask.keys = want_keys ? &keys : nullptr; ask.mix = mix;
    PassOut out; out.mean = om; out.var = ov; out.cov = oc; out.info = oi;
    return predict_core(c, run, bt, jp, ask, out);
  };
  if (!D.packed()) return core(out_mean, out_var, out_cov, out_info);
  std::vector<double> umean(mix ? 0 : (size_t)U * m), uvar(mix ? 0 : (size_t)U * m), ucov(out_cov ? (size_t)U * m * m : 0);
  std::vector<int32_t> uinfo((size_t)U, 0);
  rc = core(mix ? nullptr : umean.data(), mix ? nullptr : uvar.data(), out_cov ? ucov.data() : nullptr, uinfo.data());
  if (rc) return rc;
  if (!mix) { D.scatter(umean.data(), out_mean, (size_t)m); D.scatter(uvar.data(), out_var, (size_t)m); }
  if (out_cov) D.scatter(ucov.data(), out_cov, (size_t)m * m);
  D.scatter(uinfo.data(), out_info);
  return AGP_OK;
}

}  // namespace

int predict_batch(agp_ctx* c, const PredQuery& q, const Particles& pp, double* out_mean, double* out_var, double* out_cov, int32_t* out_info) {
  const int64_t n = q.n, m = q.m;
  const int P = pp.P;
  const double* ts_pred = q.ts_pred; const double* mean_train = q.mean_train; const double* mean_pred = q.mean_pred;
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (P < 0 || n < 0 || m < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (P == 0 || m == 0) return AGP_OK;
  if (!pp.complete() || !ts_pred || !out_mean || !out_var) return fail(c, AGP_ERR_ARG, "null pointer argument");
  if (const int rc = check_resident(c, n)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  // Structured pass (no dense factor; toeplitz_predict_sweep): marginal predictions, the n training points
  // consecutive grid points, every query one of them or a grid point after them, nothing resident to start from — the Toeplitz +
  // rank-2 particles of the call go there, the others (and any particle the recursion refuses) through the dense path below.
  if (!out_cov && !tl_in_tpredict && c->grad_struct && c->lag_contig && n >= 256 && n <= 2048 &&
      // (with factors resident, starting from them costs (n / 2048)^3 x ~14 ms of L^-T per 256 particles: the two sequential passes of
      // the structured sweep, ~3.8 us per point, are cheaper from n ~ 768 on)
      (!(c->predict_reuse && c->store.n_slots > 0) || n >= 768) && (int64_t)c->h_rank.size() >= n) {
    PredLattice plq;
    predict_lattice(c, n, ts_pred, m, plq);
    int32_t lo = 0, hi = 0;
    bool ok = plq.on;
    if (ok) {
      lo = hi = plq.rank[0];
      for (int64_t i = 1; i < n; ++i) { lo = std::min(lo, plq.rank[(size_t)i]); hi = std::max(hi, plq.rank[(size_t)i]); }
      ok = (int64_t)hi - lo + 1 == n;
    }
    std::vector<int32_t> qkind((size_t)m);
    std::vector<double> xq((size_t)m, 0.0), xres;          // xres: x - mean_train in sorted order (mean functions)
    int mF = 0;
    if (ok) {
      const int n1_pad = round_up(n, NB);
      std::vector<int32_t> at((size_t)n);          // sorted position -> training index
      for (int64_t i = 0; i < n; ++i) at[(size_t)(plq.rank[(size_t)i] - lo)] = (int32_t)i;
      for (int64_t j = 0; j < m && ok; ++j) {
        const int32_t r = plq.rank[(size_t)n1_pad + j];
        if (r < lo) { ok = false; break; }          // (a point before the series: the dense path)
        // (observed = the SAME time value, as the reference's WhiteNoise t1 == t2, src/GP.jl:135, and the dense path's split_queries: a
        // query a few ulp off a training time is a lattice point by the tolerance but not that observation -> dense path)
        if (r <= hi && ts_pred[j] != c->h_ts[(size_t)at[(size_t)(r - lo)]]) { ok = false; break; }
        if (r <= hi) { const int32_t i = at[(size_t)(r - lo)]; qkind[(size_t)j] = r - lo; xq[(size_t)j] = c->h_xs[(size_t)i] - (mean_train ? mean_train[i] : 0.0); }
        else { const int f = r - hi - 1; qkind[(size_t)j] = -1 - f; mF = std::max(mF, f + 1); }
      }
      ok = ok && n + mF <= STRUCT_JOINT_MAX && n + mF <= (int64_t)plq.rank_units * 256;
      if (ok && mean_train) {
        xres.resize((size_t)n);
        for (int64_t u = 0; u < n; ++u) { const int32_t i = at[(size_t)u]; xres[(size_t)u] = c->h_xs[(size_t)i] - mean_train[i]; }
      }
    }
    std::vector<int> part[2];
    if (ok) {
      ok = offsets_sane(pp);
      for (int p = 0; p < P && ok; ++p) ok = pp.n_ops(p) <= AGP_MAX_OPS_DEV;
      if (ok) for (int p = 0; p < P; ++p) part[toeplitz_class(pp.program(p), pp.n_ops(p)) ? 1 : 0].push_back(p);
    }
    // (two sequential passes over the joint grid: ~1.2 us per point + ~1 us per training point, whatever the class's size)
    if (ok && (int)part[1].size() >= STRUCT_PRED_MIN_CLASS) {
      const int32_t rank0_abs = c->h_rank[0] - (plq.rank[0] - lo);          // rank of the first training point in the resident series
      // (noise_pred defaults to noise in the sub-batches)
      Particles ppn = pp;
      if (!ppn.noise_pred) ppn.noise_pred = pp.noise;
      SubBatch sT, sD;
      pack_particles(part[1], ppn, sT);
      std::vector<double> tmean(part[1].size() * (size_t)m), tvar(part[1].size() * (size_t)m), dmean, dvar;
      std::vector<int32_t> tinfo(part[1].size(), 0), dinfo;
      Beside side([&] {
        return toeplitz_predict_sweep(c, q, sT.view(), rank0_abs, mF, plq, qkind, xq, tmean.data(), tvar.data(), tinfo.data(),
                                       mean_train ? xres.data() : nullptr);
      });
      auto dense = [&](const std::vector<int>& ix) {
        if (ix.empty()) return 0;
        pack_particles(ix, ppn, sD);
        dmean.resize(ix.size() * (size_t)m); dvar.resize(ix.size() * (size_t)m); dinfo.assign(ix.size(), 0);
        TlFlag nested(tl_in_tpredict);
        const int rc0 = predict_batch(c, q, sD.view(), dmean.data(), dvar.data(), nullptr, dinfo.data());
        if (rc0) return rc0;
        for (size_t b = 0; b < ix.size(); ++b) {
          std::memcpy(out_mean + (size_t)ix[b] * m, dmean.data() + b * (size_t)m, sizeof(double) * (size_t)m);
          std::memcpy(out_var + (size_t)ix[b] * m, dvar.data() + b * (size_t)m, sizeof(double) * (size_t)m);
          if (out_info) out_info[ix[b]] = dinfo[b];
        }
        return 0;
      };
      const int rcD = dense(part[0]);
      const int rcT = side.join();
      if (rcD) return rcD;
      if (rcT) return rcT;
      std::vector<int> refused;
      int64_t done = 0;
      for (size_t b = 0; b < part[1].size(); ++b) {
        if (tinfo[b] != 0) { refused.push_back(part[1][b]); continue; }
        std::memcpy(out_mean + (size_t)part[1][b] * m, tmean.data() + b * (size_t)m, sizeof(double) * (size_t)m);
        std::memcpy(out_var + (size_t)part[1][b] * m, tvar.data() + b * (size_t)m, sizeof(double) * (size_t)m);
        if (out_info) out_info[part[1][b]] = 0;
        ++done;
      }
      { std::lock_guard<std::mutex> g(c->mu); c->n_struct_pred += done; }
      return dense(refused);
    }
  }
  return predict_dense(c, q, pp, out_mean, out_var, out_cov, out_info, nullptr, nullptr);
}

int predict_joint_batch(agp_ctx* c, const PredQuery& q, const double* y_pred, const Particles& pp, double* out_logpdf, int32_t* out_info,
                        JointHooks* hooks) {
  HIPCHK(c, hipSetDevice(c->device));
  // identical particles (a resampled population, src/inference_smc_anneal_data.jl:198-204) are evaluated once, as in agp_predict_batch
  // (malformed offsets, c->dedup off: every particle — compile_batch diagnoses the offsets)
  const Distinct D(pp, c->dedup != 0);
  const int U = D.U();
  std::vector<double> ulp((size_t)U);
  std::vector<int32_t> uinfo((size_t)U, 0);
  PredLattice pl;
  predict_lattice(c, q.n, q.ts_pred, q.m, pl);
  Batch bt;
  CompileOpts co;
  co.fuse_hint = co.flow_limit = c->flow != 0;      // (predict_logpdf_core's schedule)
  co.lag = pl.on; co.lag_units = pl.on ? pl.rank_units : 1; co.rank_extra = pl.on;
  int rc = compile_batch(c, D.run(), bt, co);
  if (rc) return rc;
  if (hooks && hooks->plan)
    if ((rc = hooks->plan(U, D.packed() ? D.rep : std::vector<int>(), bt.order))) return rc;
  JointPlan jp;
  plan_joint(c, q, true, false, nullptr, &pl, jp);      // (the whole of Sigma*: no split)
  rc = predict_logpdf_core(c, jp, y_pred, D.run(), bt, ulp.data(), uinfo.data(), hooks);
  if (rc) return rc;
  D.scatter(ulp.data(), out_logpdf); D.scatter(uinfo.data(), out_info);
  return AGP_OK;
}

int predict_mixture_cov(agp_ctx* c, const PredQuery& q, const Particles& pp, const double* weights, MixPass& mp, int32_t* out_info) {
  HIPCHK(c, hipSetDevice(c->device));
  return predict_dense(c, q, pp, nullptr, nullptr, nullptr, out_info, weights, &mp);
}

namespace {

// infer_gp_sum for a population (agp_infer_gp_sum_batch) and predict_sum's numbers (agp_predict_sum_batch, sp->readout): particle
// pp's M components are the CSR entries [pp M, (pp + 1) M) of `comp` (comp.P particles; noises per particle).  Each particle's composite
// program is the single entry's; identical particles (program, parameters, noise, noise_pred: a resampled population) run once;
// predict_core runs the batch with codes, the single entry's diagonal terms (noise_pred on the observable rows only, see SumPass) and
// the pinned schedule.
int sum_batch_body(agp_ctx* c, int64_t n, const double* ts_pred, int64_t p, int32_t M, const Particles& comp, double* out_mean,
                   double* out_var, double* out_cov, int32_t* out_info, SumPass* sp) {
  const int P = comp.P;
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (P < 1) return fail(c, AGP_ERR_ARG, "P must be >= 1");
  if (M < 1 || M > 200) return fail(c, AGP_ERR_ARG, "M must be in 1..200");
  if (p < 0 || n < 0) return fail(c, AGP_ERR_ARG, "negative size");
  if (const int rc = check_resident(c, n)) return rc;
  const int64_t nq = (int64_t)sp->z.size();
  const int64_t ma = (int64_t)(M + 1) * p;
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)P * ma >= lim || (out_cov && ma > 0 && (int64_t)P * ma >= lim / ma) || (nq > 0 && (int64_t)P * ma >= lim / nq))
    return fail(c, AGP_ERR_ARG, "an output exceeds 2^31 elements");
  if (p == 0) return AGP_OK;
  if (!comp.complete() || !ts_pred || !out_mean || (!sp->readout && !out_var) || (nq > 0 && !sp->out_x))
    return fail(c, AGP_ERR_ARG, "null pointer argument");
  HIPCHK(c, hipSetDevice(c->device));
  // composite programs, per particle (as agp_infer_gp_sum)
  std::vector<int32_t> coff((size_t)P + 1, 0), cpoff((size_t)P + 1, 0);
  std::vector<uint8_t> cops; std::vector<double> cprm;
  char buf[256];
  std::string err;
  for (int32_t pp = 0; pp < P; ++pp) {
    if (const int rc = append_composite(comp, (int64_t)pp * M, M, AGP_MAX_OPS, cops, cprm, err)) {
      snprintf(buf, sizeof buf, "particle %d: ", (int)pp);
      return fail(c, rc, buf + err);
    }
    coff[(size_t)pp + 1] = (int32_t)cops.size(); cpoff[(size_t)pp + 1] = (int32_t)cprm.size();
  }
  // noise_pred NULL: each particle's own noise (src/GP.jl:913)
  const double* npv = comp.noise_pred ? comp.noise_pred : comp.noise;
  // (always packed: predict_core reads the packed arrays whatever the population; `copies` decides where it writes)
  const Distinct D({P, coff.data(), cops.data(), cpoff.data(), cprm.data(), comp.noise, npv}, c->dedup != 0, Distinct::Pack::always);
  const Particles run = D.run();
  const int U = D.U();
  const bool copies = D.copies();
  { std::lock_guard<std::mutex> g(c->mu); c->n_particles_seen += P; c->n_particles_run += U; }      // (agp_get_dedup_stats)
  // query points: F_1(T*) ... F_M(T*) (codes 1..M), then X(T*) (code 0); JITTER on every row (noise_pred: k_pred_extract)
  std::vector<double> tq((size_t)ma), dadd((size_t)ma, 1e-8);
  std::vector<uint8_t> code((size_t)ma);
  for (int i = 0; i <= M; ++i)
    for (int64_t j = 0; j < p; ++j) {
      tq[(size_t)i * p + j] = ts_pred[j];
      code[(size_t)i * p + j] = (uint8_t)(i < M ? i + 1 : 0);
    }
  Batch bt;
  CompileOpts co;
  co.allow_sel = true; co.fuse_hint = co.flow_limit = c->flow != 0;      // (predict_core's schedule for this pass)
  int rc = compile_batch(c, run, bt, co);
  if (rc) {
    // name the caller's particle: the first distinct particle that does not compile on its own
    CompileOpts c1;
    c1.allow_sel = true;
    for (int u = 0; u < U; ++u) {
      Batch b1;
      const int32_t o1[2] = {0, run.n_ops(u)}, q1[2] = {0, run.n_prm(u)};
      const double zero = 0.0;
      if (compile_batch(c, {1, o1, run.program(u), q1, q1[1] > 0 ? run.params(u) : &zero, nullptr, nullptr}, b1, c1) == 0) continue;
      std::string e;
      { std::lock_guard<std::mutex> g(c->mu); e = c->err; }
      if (e.rfind("particle 0: ", 0) == 0) e = e.substr(12);
      snprintf(buf, sizeof buf, "particle %d: ", D.uniq[(size_t)u]);
      return fail(c, AGP_ERR_PROGRAM, buf + e);
    }
    return rc;
  }
  const size_t ue = (size_t)ma;
  std::vector<double> umean(copies ? U * ue : 0), uvar(copies && out_var ? U * ue : 0), ucov(copies && out_cov ? U * ue * ue : 0),
      ux(copies && nq > 0 ? U * ue * (size_t)nq : 0);
  std::vector<int32_t> uinfo((size_t)U, 0);
  double* x_caller = sp->out_x;
  if (copies && nq > 0) sp->out_x = ux.data();
  JointPlan jp;
  plan_joint(c, {n, tq.data(), ma, nullptr, nullptr}, out_cov != nullptr, true, dadd.data(), nullptr, jp);
  PassAsk ask; ask.pred_code = code.data(); ask.diag_add = dadd.data(); ask.sum = sp;
  PassOut out; out.mean = copies ? umean.data() : out_mean; out.var = copies ? (out_var ? uvar.data() : nullptr) : out_var;
  out.cov = copies ? (out_cov ? ucov.data() : nullptr) : out_cov; out.info = uinfo.data();
  rc = predict_core(c, run, bt, jp, ask, out);
  sp->out_x = x_caller;
  if (rc) return rc;
  D.scatter(uinfo.data(), out_info);
  if (!copies) return AGP_OK;
  D.scatter(umean.data(), out_mean, ue);
  if (out_var) D.scatter(uvar.data(), out_var, ue);
  if (out_cov) D.scatter(ucov.data(), out_cov, ue * ue);
  if (nq > 0) D.scatter(ux.data(), x_caller, ue * (size_t)nq);
  return AGP_OK;
}

}  // namespace

extern "C" {

int agp_predict_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, int32_t P,
                      const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                      const double* noise, const double* noise_pred, const double* mean_train,
                      const double* mean_pred, double* out_mean, double* out_var, double* out_cov,
                      int32_t* out_info) {
  return abi_guard(c, [&] {
    return predict_batch(c, {n, ts_pred, m, mean_train, mean_pred}, {P, op_off, ops, prm_off, prm, noise, noise_pred}, out_mean, out_var,
                         out_cov, out_info);
  });
}

int agp_predict_logpdf_batch(agp_ctx* c, int64_t n, const double* ts_pred, const double* y_pred, int64_t m, int32_t P,
                             const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                             const double* noise, const double* noise_pred, const double* mean_train, const double* mean_pred,
                             double* out_logpdf, int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    const Particles pp{P, op_off, ops, prm_off, prm, noise, noise_pred};
    if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
    if (P < 0 || n < 0 || m < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if (const int rc = check_resident(c, n)) return rc;
    if (P == 0) return AGP_OK;
    if (!out_logpdf) return fail(c, AGP_ERR_ARG, "null pointer argument");
    if (m == 0) {
      // the empty vector has density 1 under every particle (the reference scores [] as 0.)
      for (int p = 0; p < P; ++p) { out_logpdf[p] = 0.0; if (out_info) out_info[p] = 0; }
      return AGP_OK;
    }
    if (!pp.complete() || !ts_pred || !y_pred) return fail(c, AGP_ERR_ARG, "null pointer argument");
    return predict_joint_batch(c, {n, ts_pred, m, mean_train, mean_pred}, y_pred, pp, out_logpdf, out_info, nullptr);
  });
}

// infer_gp_sum (src/GP.jl:904-993): posterior over Z = [F_1(T*); ...; F_M(T*); X(T*)] given X(T) = xs, for the
// sum-of-GPs model X = sum_i F_i + noise.  The joint prior covariance over [X(T); Z] is the single program
// sum_i SEL_i * K_i evaluated on coded points (SEL_i(a,b) = 1 when both points are the observable or the
// latent of component i), so the whole computation is one pass of the predictive machinery:
// Cholesky of Sigma_bb = S_tt + noise I (src/GP.jl:982), Schur complement (984), + JITTER I (986).
int agp_infer_gp_sum(agp_ctx* c, int64_t n, const double* ts_pred, int64_t p, int32_t M,
                     const int32_t* op_off, const uint8_t* ops, const int32_t* prm_off, const double* prm,
                     double noise, double noise_pred, double* out_mean, double* out_cov, int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
    if (n < 0 || p <= 0 || M <= 0 || M > 200) return fail(c, AGP_ERR_ARG, "bad sizes");
    if (!op_off || !ops || !prm_off || !prm || !ts_pred || !out_mean) return fail(c, AGP_ERR_ARG, "null pointer argument");
    if (const int rc = check_resident(c, n)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // (every opcode is checked before the length, as this entry always has)
    std::vector<uint8_t> cops; std::vector<double> cprm;
    std::string err;
    if (const int rc = append_composite({M, op_off, ops, prm_off, prm, nullptr, nullptr}, 0, M, INT32_MAX, cops, cprm, err)) return fail(c, rc, err);
    if ((int)cops.size() > AGP_MAX_OPS) return fail(c, AGP_ERR_PROGRAM, "composite program too long");
    const int32_t coff[2] = {0, (int32_t)cops.size()}, cpoff[2] = {0, (int32_t)cprm.size()};
    const double zero = 0.0;
    const Particles one{1, coff, cops.data(), cpoff, cprm.data(), &noise, &zero};
    Batch bt;
    CompileOpts co;
    co.allow_sel = true;
    int rc = compile_batch(c, one, bt, co);
    if (rc) return rc;
    // query points: F_1(T*) ... F_M(T*) (codes 1..M), then X(T*) (code 0)
    const int64_t ma = (int64_t)(M + 1) * p;
    std::vector<double> tq((size_t)ma), dadd((size_t)ma), var((size_t)ma);
    std::vector<uint8_t> code((size_t)ma);
    for (int i = 0; i <= M; ++i)
      for (int64_t j = 0; j < p; ++j) {
        const size_t g = (size_t)i * p + j;
        tq[g] = ts_pred[j];
        code[g] = (uint8_t)(i < M ? i + 1 : 0);
        dadd[g] = 1e-8 + (i == M ? noise_pred : 0.0);       // JITTER (src/GP.jl:760,986) + noise_pred on X(T*)
      }
    int32_t info = 0;
    JointPlan jp;
    plan_joint(c, {n, tq.data(), ma, nullptr, nullptr}, out_cov != nullptr, true, dadd.data(), nullptr, jp);
    PassAsk ask; ask.pred_code = code.data(); ask.diag_add = dadd.data();
    PassOut out; out.mean = out_mean; out.var = var.data(); out.cov = out_cov; out.info = &info;
    rc = predict_core(c, one, bt, jp, ask, out);
    if (out_info) *out_info = info;
    return rc;
  });
}

int agp_infer_gp_sum_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t p, int32_t P, int32_t M, const int32_t* op_off,
                           const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise, const double* noise_pred,
                           double* out_mean, double* out_var, double* out_cov, int32_t* out_info) {
  SumPass sp;      // (no read-out: the pinned schedule and the observable-rows noise_pred only)
  sp.p_rows = p;
  return abi_guard(c, [&] {
    return sum_batch_body(c, n, ts_pred, p, M, {P, op_off, ops, prm_off, prm, noise, noise_pred}, out_mean, out_var, out_cov, out_info, &sp);
  });
}

int agp_predict_sum_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t p, int32_t P, int32_t M, const int32_t* op_off,
                          const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise, const double* noise_pred,
                          double y_slope, double y_intercept, const double* q, int64_t nq, double* out_mean, double* out_x,
                          int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
    if (nq < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if (nq > 0 && !q) return fail(c, AGP_ERR_ARG, "null q");
    for (int64_t k = 0; k < nq; ++k)
      if (!(q[k] > 0.0 && q[k] < 1.0)) return fail(c, AGP_ERR_ARG, "quantile must be in (0, 1)");
    if (const int rc = check_y_transform(c, y_slope, y_intercept)) return rc;
    SumPass sp;
    sp.readout = true; sp.p_rows = p; sp.slope = y_slope; sp.intercept = y_intercept; sp.out_x = out_x;
    sp.z.resize((size_t)nq);
    for (int64_t k = 0; k < nq; ++k) sp.z[(size_t)k] = ndtri(q[k]);
    return sum_batch_body(c, n, ts_pred, p, M, {P, op_off, ops, prm_off, prm, noise, noise_pred}, out_mean, nullptr, nullptr, out_info, &sp);
  });
}

int agp_cov_matrix(agp_ctx* c, const double* ts, int64_t n, const uint8_t* ops, int32_t n_ops, const double* prm,
                   int32_t n_prm, double noise, double* out_K) {
  return abi_guard(c, [&]() -> int {
    if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
    if (n < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if (n == 0) return AGP_OK;
    if (!ts || !ops || !out_K) return fail(c, AGP_ERR_ARG, "null pointer argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int32_t op_off[2] = {0, n_ops}, prm_off[2] = {0, n_prm};
    double dummy = 0.0;
    Batch bt;
    int rc = compile_batch(c, {1, op_off, ops, prm_off, prm ? prm : &dummy, &noise, nullptr}, bt);
    if (rc) return rc;
    SlotGuard sg(c);
    Slot* s = sg.s;
    if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    hipStream_t st = s->stream;
    const int n_pad = round_up(n, NB), nt = n_pad / NB, ntiles = nt * (nt + 1) / 2;
    const long long strideA = (long long)ntiles * NB2;
    std::vector<double> tt((size_t)n_pad, 0.0);
    std::copy(ts, ts + n, tt.begin());
    HIPCHK(c, s->A.ensure((size_t)strideA * 8));
    HIPCHK(c, s->hdr.ensure(sizeof(ProgHdr)));
    HIPCHK(c, s->ops.ensure(bt.ops.size()));
    HIPCHK(c, s->prm.ensure(sizeof(double) * std::max<size_t>(1, bt.prm.size())));
    HIPCHK(c, s->noise.ensure(sizeof(double)));
    HIPCHK(c, s->tt.ensure(sizeof(double) * (size_t)n_pad));
    HIPCHK(c, s->dense.ensure(sizeof(double) * (size_t)n * n));
    HIPCHK(c, hipMemcpyAsync(s->hdr.p, bt.hdr.data(), sizeof(ProgHdr), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->ops.p, bt.ops.data(), bt.ops.size(), hipMemcpyHostToDevice, st));
    if (!bt.prm.empty())
      HIPCHK(c, hipMemcpyAsync(s->prm.p, bt.prm.data(), sizeof(double) * bt.prm.size(), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->noise.p, &noise, sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(s->tt.p, tt.data(), sizeof(double) * n_pad, hipMemcpyHostToDevice, st));
    CovArgs cv = {};
    cv.tt = s->tt.as<double>(); cv.n1 = (int)n; cv.n1_pad = n_pad; cv.m2 = 0; cv.nt = nt;
    cv.hdr = s->hdr.as<ProgHdr>(); cv.ops = s->ops.as<uint8_t>(); cv.prm = s->prm.as<double>();
    cv.noise = s->noise.as<double>(); cv.A = s->A.as<double>(); cv.strideA = strideA; cv.P = 1;
    cv.p_off = 0;
    HIPCHK(c, launch_cov(st, cv, ntiles, 1, bt.max_cp, bt.max_depth, bt.max_ops));
    const long long nel = (long long)n * n;
    launch_unpack_dense(st, s->A.as<double>(), (int)n, 0, s->dense.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out_K, s->dense.p, sizeof(double) * nel, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return AGP_OK;
  });
}

int agp_debug_cholesky(agp_ctx* c, const double* K, int64_t n, double* out_L, int32_t* out_info) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (n <= 0 || !K || !out_L) return fail(c, AGP_ERR_ARG, "bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const int n_pad = round_up(n, NB), nt = n_pad / NB, ntiles = nt * (nt + 1) / 2;
  const long long strideA = (long long)ntiles * NB2;
  const long long nel = (long long)n * n;
  HIPCHK(c, s->A.ensure((size_t)strideA * 8));
  HIPCHK(c, s->W.ensure(sizeof(double) * NSB * 256));
  HIPCHK(c, s->vec.ensure(sizeof(double) * (size_t)n_pad));
  HIPCHK(c, s->partial.ensure(sizeof(double) * 2 * (size_t)nt));
  HIPCHK(c, s->info.ensure(sizeof(int)));
  HIPCHK(c, s->dense.ensure(sizeof(double) * (size_t)nel));
  HIPCHK(c, hipMemcpyAsync(s->dense.p, K, sizeof(double) * nel, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(s->vec.p, 0, sizeof(double) * n_pad, st));
  HIPCHK(c, hipMemsetAsync(s->info.p, 0, sizeof(int), st));
  HIPCHK(c, s->ready.ensure(sizeof(int)));
  HIPCHK(c, hipMemsetAsync(s->ready.p, 0, sizeof(int), st));
  launch_pack_dense(st, s->dense.as<double>(), (int)n, nt, strideA, s->A.as<double>());
  CholArgs ca = {};
  ca.A = s->A.as<double>(); ca.strideA = strideA; ca.W = s->W.as<double>(); ca.vec = s->vec.as<double>();
  ca.ldv = n_pad; ca.partial = s->partial.as<double>(); ca.info = s->info.as<int>(); ca.P = 1; ca.nt = nt;
  ca.k = 0; ca.nt1 = nt;
  ca.tt = nullptr; ca.hdr = nullptr; ca.ops = nullptr; ca.prm = nullptr; ca.noise = nullptr; ca.n1 = ca.n1_pad = ca.m2 = 0; ca.n_fused = 0; ca.ready = s->ready.as<int>();
  HIPCHK(c, run_factor(st, ca, nt, 0, nullptr, nullptr, use_split_diag(c, ca.P)));
  launch_unpack_dense(st, s->A.as<double>(), (int)n, 1, s->dense.as<double>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out_L, s->dense.p, sizeof(double) * nel, hipMemcpyDeviceToHost, st));
  if (out_info) HIPCHK(c, hipMemcpyAsync(out_info, s->info.p, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  return AGP_OK;
}

// Factor P caller-supplied matrices with ONE chosen schedule and hand back everything the diagonal tiles produce (see
// include/autogp_hip.h).  The schedules are the sweeps' own host functions (run_factor, launch_joint_flow) and predicates
// (use_flow, use_split_diag, use_right_looking, hybrid_switch_column): nothing of a schedule is restated here.
int agp_debug_factor_batch(agp_ctx* c, const double* K, const double* y, int64_t n, int32_t P, int32_t schedule,
                           double* out_L, double* out_beta, double* out_partial, int32_t* out_info) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  if (n <= 0 || P <= 0 || !K || !out_L || !out_info) return fail(c, AGP_ERR_ARG, "bad arguments");
  if (schedule < -1 || schedule > 4) return fail(c, AGP_ERR_ARG, "unknown schedule (-1 .. 4)");
  if (n > 8192 || (int64_t)P * n * n > ((int64_t)1 << 28)) return fail(c, AGP_ERR_ARG, "debug probe: batch too large");
  HIPCHK(c, hipSetDevice(c->device));
  const int n_pad = round_up(n, NB), nt = n_pad / NB, ntiles = nt * (nt + 1) / 2;
  if (schedule == 3 && hybrid_switch_column(P, nt, nt, HYBRID_BLOCKS) >= nt)
    return fail(c, AGP_ERR_ARG, "hybrid schedule: no switch column for this (P, nt); it would run the mixed launches throughout");
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const long long strideA = (long long)ntiles * NB2;
  const long long nel = (long long)n * n;
  const int wsteps = nt;      // every block column keeps its inverse blocks, as in the sweeps with the dataflow schedule admitted
  HIPCHK(c, s->A.ensure(sizeof(double) * (size_t)strideA * P));
  HIPCHK(c, s->W.ensure(sizeof(double) * NSB * 256 * (size_t)P * wsteps));
  HIPCHK(c, s->vec.ensure(sizeof(double) * (size_t)n_pad * P));
  HIPCHK(c, s->partial.ensure(sizeof(double) * 2 * (size_t)nt * P));
  HIPCHK(c, s->info.ensure(sizeof(int) * (size_t)P));
  HIPCHK(c, s->ready.ensure(sizeof(int) * (size_t)P));
  HIPCHK(c, s->dense.ensure(sizeof(double) * (size_t)nel * P));
  HIPCHK(c, hipMemcpyAsync(s->dense.p, K, sizeof(double) * nel * P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(s->vec.p, 0, sizeof(double) * (size_t)n_pad * P, st));
  if (y)
    HIPCHK(c, hipMemcpy2DAsync(s->vec.p, sizeof(double) * n_pad, y, sizeof(double) * n, sizeof(double) * n, P, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(s->info.p, 0, sizeof(int) * (size_t)P, st));
  HIPCHK(c, hipMemsetAsync(s->ready.p, 0, sizeof(int) * (size_t)P, st));
  for (int p = 0; p < P; ++p)
    launch_pack_dense(st, s->dense.as<double>() + (size_t)p * nel, (int)n, nt, strideA, s->A.as<double>() + (size_t)p * strideA);
  HIPCHK(c, hipGetLastError());
  CholArgs ca = {};
  ca.A = s->A.as<double>(); ca.strideA = strideA; ca.W = s->W.as<double>(); ca.wsteps = wsteps; ca.vec = s->vec.as<double>();
  ca.ldv = n_pad; ca.partial = s->partial.as<double>(); ca.info = s->info.as<int>(); ca.P = P; ca.nt = nt;
  ca.k = 0; ca.nt1 = nt; ca.ready = s->ready.as<int>();      // (n1 = 0: dense input, the padding is factored like data; n_fused = 0)
  bool flow = schedule == 4, split = schedule == 1, rl = schedule == 2;
  int hybrid = schedule == 3 ? HYBRID_BLOCKS : 0;
  if (schedule < 0) {      // logpdf_batch_impl's choice for a batch without resident factors
    flow = use_flow(c, P, nt); split = use_split_diag(c, P); rl = use_right_looking(c, P); hybrid = HYBRID_BLOCKS;
  }
  if (flow) {
    int rc = launch_joint_flow(c, s, st, ca, 0, wsteps);
    if (rc) return rc;
  } else {
    HIPCHK(c, run_factor(st, ca, nt, 0, nullptr, nullptr, split, rl, hybrid));
  }
  for (int p = 0; p < P; ++p)
    launch_unpack_dense(st, s->A.as<double>() + (size_t)p * strideA, (int)n, 1, s->dense.as<double>() + (size_t)p * nel);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out_L, s->dense.p, sizeof(double) * nel * P, hipMemcpyDeviceToHost, st));
  if (out_beta)
    HIPCHK(c, hipMemcpy2DAsync(out_beta, sizeof(double) * n, s->vec.p, sizeof(double) * n_pad, sizeof(double) * n, P, hipMemcpyDeviceToHost, st));
  std::vector<double> part((size_t)2 * nt * P);
  HIPCHK(c, hipMemcpyAsync(part.data(), s->partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipMemcpyAsync(out_info, s->info.p, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (out_partial)
    for (int p = 0; p < P; ++p) {      // block columns in k_finish_logpdf's order
      double ld = 0.0, ss = 0.0;
      for (int k = 0; k < nt; ++k) { ld += part[((size_t)p * nt + k) * 2]; ss += part[((size_t)p * nt + k) * 2 + 1]; }
      out_partial[2 * p] = ld; out_partial[2 * p + 1] = ss;
    }
  return AGP_OK;
}

int agp_debug_mfma_peak(agp_ctx* c, int32_t iters, int32_t wg_per_cu, double* out_tflops, double* out_ghz) {
  if (!c || !out_tflops || !out_ghz) return fail(c, AGP_ERR_ARG, "null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  hipDeviceProp_t prop;
  HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
  const int mode = wg_per_cu >> 8;          // (high bits: what the waves execute, see k_mfma_peak)
  wg_per_cu &= 255;
  const int nblk = prop.multiProcessorCount * (wg_per_cu > 0 ? wg_per_cu : 2);
  double* d_out = nullptr; long long* d_cyc = nullptr;
  HIPCHK(c, malloc_values(c->poison, (void**)&d_out, sizeof(double) * 256 * (size_t)nblk));
  HIPCHK(c, hipMalloc((void**)&d_cyc, sizeof(long long) * (size_t)nblk));
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
  launch_mfma_peak(nblk, d_out, d_cyc, 64, mode);   // warm-up
  HIPCHK(c, hipEventRecord(e0, 0));
  launch_mfma_peak(nblk, d_out, d_cyc, iters, mode);
  HIPCHK(c, hipEventRecord(e1, 0));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  std::vector<long long> cyc(nblk);
  HIPCHK(c, hipMemcpy(cyc.data(), d_cyc, sizeof(long long) * nblk, hipMemcpyDeviceToHost));
  double mean_cyc = 0; for (auto v : cyc) mean_cyc += (double)v; mean_cyc /= nblk;
  const double flops = (double)nblk * 4.0 * 16.0 * (double)iters * 2048.0;
  *out_tflops = flops / (ms * 1e-3) / 1e12;
  *out_ghz = mean_cyc / (ms * 1e-3) / 1e9;     // shader cycles per second while the kernel ran
  (void)hipFree(d_out); (void)hipFree(d_cyc); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return AGP_OK;
}

// ---- measurement build only (-DAGP_EXPERIMENTS -> libautogp_hip_exp.so; declared in csrc/experiments/agp_experiments_abi.h) ----
#ifdef AGP_EXPERIMENTS
int agp_debug_gemm_variant(agp_ctx* c, int32_t P, int32_t nt, int32_t k, int32_t variant, int32_t reps, double* out_ms) {
  if (!c || !out_ms || P <= 0 || nt < 2 || k < 1 || k >= nt - 0) return fail(c, AGP_ERR_ARG, "bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  SlotGuard sg(c);
  Slot* s = sg.s;
  if (!s->stream) HIPCHK(c, hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  hipStream_t st = s->stream;
  const int ntiles = nt * (nt + 1) / 2;
  const long long strideA = (long long)ntiles * NB2;
  HIPCHK(c, s->A.ensure((size_t)strideA * 8 * P));
  hipLaunchKernelGGL(k_fill_pseudo, dim3(4096), dim3(256), 0, st, s->A.as<double>(), strideA * P);
  CholArgs ca = {};
  ca.A = s->A.as<double>(); ca.strideA = strideA; ca.W = nullptr; ca.vec = nullptr; ca.ldv = 0; ca.partial = nullptr;
  ca.info = nullptr; ca.P = P; ca.nt = nt; ca.k = k; ca.nt1 = nt; ca.tiles = nt - k - 1;
  if (ca.tiles < 1) return fail(c, AGP_ERR_ARG, "no off-diagonal tiles");
  const int grid = 8 * ((P + 7) / 8) * ca.tiles;
  hipEvent_t e0, e1;
  HIPCHK(c, hipEventCreate(&e0)); HIPCHK(c, hipEventCreate(&e1));
  const int Pg8 = 8 * ((P + 7) / 8);
  for (int r = 0; r < reps + 1; ++r) {
    if (r == 1) HIPCHK(c, hipEventRecord(e0, st));
    switch (variant) {
      case 2000: {   // every block column 1..nt-2 in ONE launch (k is ignored)
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * (nt - kk - 1);
        hipLaunchKernelGGL((k_gemm_strip<16, true, true>), dim3(blocks), dim3(256), 0, st, ca);
        break;
      }
      case 2002: {   // as 2000 with twice the prefetch distance
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * (nt - kk - 1);
        hipLaunchKernelGGL((k_gemm_strip<16, true, true, true>), dim3(blocks), dim3(256), 0, st, ca);
        break;
      }
      case 2003: {   // as 2000 without LDS / barriers: both operands global -> registers
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * (nt - kk - 1);
        hipLaunchKernelGGL((k_gemm_nolds<true>), dim3(blocks), dim3(256), 0, st, ca);
        break;
      }
      case 4000: case 4032: {   // 256 x 128 macro-items (two row tiles per workgroup, one workgroup per CU), every block column in one launch
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * ((nt - kk) / 2);
        if (variant == 4000) hipLaunchKernelGGL((k_gemm_macro<true, 16>), dim3(blocks), dim3(256), 0, st, ca);
        else hipLaunchKernelGGL((k_gemm_macro<true, 32>), dim3(blocks), dim3(256), 0, st, ca);
        break;
      }
      case 4100: {   // 256 x 128 macro-items, eight waves (two row tiles per workgroup share the column slab in LDS), one launch
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * ((nt - kk) / 2);
        hipLaunchKernelGGL((k_gemm_pair8<true>), dim3(blocks), dim3(512), 0, st, ca);
        break;
      }
      case 3000: {   // every block column in one launch, EIGHT waves per workgroup (column halves)
        int blocks = 0;
        for (int kk = 1; kk < nt - 1; ++kk) blocks += Pg8 * (nt - kk - 1);
        hipLaunchKernelGGL((k_gemm_strip8<16, true>), dim3(blocks), dim3(512), 0, st, ca);
        break;
      }
      case 3001: {   // one launch per block column, eight waves per workgroup
        CholArgs cb = ca;
        for (int kk = 1; kk < nt - 1; ++kk) {
          cb.k = kk; cb.tiles = nt - kk - 1;
          hipLaunchKernelGGL((k_gemm_strip8<16, false>), dim3(Pg8 * cb.tiles), dim3(512), 0, st, cb);
        }
        break;
      }
      case 3032: {   // as 3001 with 32-column slabs
        CholArgs cb = ca;
        for (int kk = 1; kk < nt - 1; ++kk) {
          cb.k = kk; cb.tiles = nt - kk - 1;
          hipLaunchKernelGGL((k_gemm_strip8<32, false>), dim3(Pg8 * cb.tiles), dim3(512), 0, st, cb);
        }
        break;
      }
      case 2001: {   // the same tiles, one launch per block column
        CholArgs cb = ca;
        for (int kk = 1; kk < nt - 1; ++kk) {
          cb.k = kk; cb.tiles = nt - kk - 1;
          hipLaunchKernelGGL((k_gemm_strip<16, true, false>), dim3(Pg8 * cb.tiles), dim3(256), 0, st, cb);
        }
        break;
      }
      case 0: launch_variant<0>(st, grid, ca); break;
      case 1: launch_variant<1>(st, grid, ca); break;
      case 3: launch_variant<3>(st, grid, ca); break;
      case 7: launch_variant<7>(st, grid, ca); break;
      case 8: launch_variant<8>(st, grid, ca); break;
      case 16: launch_variant<16>(st, grid, ca); break;
      case 19: launch_variant<19>(st, grid, ca); break;
      case 23: launch_variant<23>(st, grid, ca); break;
      case 24: launch_variant<24>(st, grid, ca); break;
      case 40: launch_variant<40>(st, grid, ca); break;
      case 104: launch_variant<104>(st, grid, ca); break;
      case 168: launch_variant<168>(st, grid, ca); break;
      case 152: launch_variant<152>(st, grid, ca); break;
      case 1016: hipLaunchKernelGGL((k_gemm_strip<16, true>), dim3(grid), dim3(256), 0, st, ca); break;
      case 1032: hipLaunchKernelGGL((k_gemm_strip<32, true>), dim3(grid), dim3(256), 0, st, ca); break;
      case 1008: hipLaunchKernelGGL((k_gemm_strip<8, true>), dim3(grid), dim3(256), 0, st, ca); break;
      default: return fail(c, AGP_ERR_ARG, "unknown variant");
    }
  }
  HIPCHK(c, hipEventRecord(e1, st));
  HIPCHK(c, hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
  *out_ms = ms / reps;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  HIPCHK(c, hipGetLastError());
  return AGP_OK;
}

// Timeline of the next dataflow sweeps (k_chol_flow): out has 4 int64 per work item — start, end (100 MHz ticks),
// ticks spent waiting for operand tiles inside the K-loop, and (workgroup << 48 | particle << 24 | tile row << 12 |
// block column).  enable: allocate for max_items and start recording; otherwise copy out what was recorded.
int agp_debug_flow_trace(agp_ctx* c, int32_t enable, int64_t max_items, int64_t* out) {
  if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  if (enable) {
    if (c->d_flow_trace) { (void)hipFree(c->d_flow_trace); c->d_flow_trace = nullptr; }
    if (max_items <= 0) { c->flow_trace_items = 0; return AGP_OK; }
    HIPCHK(c, hipMalloc((void**)&c->d_flow_trace, sizeof(long long) * 8 * (size_t)max_items));
    HIPCHK(c, hipMemset(c->d_flow_trace, 0, sizeof(long long) * 8 * (size_t)max_items));
    c->flow_trace_items = (size_t)max_items;
    return AGP_OK;
  }
  if (!out || !c->d_flow_trace || (size_t)max_items > c->flow_trace_items) return fail(c, AGP_ERR_ARG, "no trace recorded");
  HIPCHK(c, hipMemcpy(out, c->d_flow_trace, sizeof(long long) * 8 * (size_t)max_items, hipMemcpyDeviceToHost));
  return AGP_OK;
}
#endif  // AGP_EXPERIMENTS

int agp_debug_math(agp_ctx* c, int32_t which, const double* x, const double* g, double* y, int32_t n) {
  if (!c || !x || !y || n <= 0 || which < 0 || which > 9 || (which == 3 && !g)) return fail(c, AGP_ERR_ARG, "bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  double *dx = nullptr, *dg = nullptr, *dy = nullptr;
  HIPCHK(c, malloc_values(c->poison, (void**)&dx, sizeof(double) * n));
  HIPCHK(c, malloc_values(c->poison, (void**)&dg, sizeof(double) * n));
  HIPCHK(c, malloc_values(c->poison, (void**)&dy, sizeof(double) * n));
  HIPCHK(c, hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
  if (g) HIPCHK(c, hipMemcpy(dg, g, sizeof(double) * n, hipMemcpyHostToDevice));
  launch_math_probe(which, dx, dg, dy, n);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpy(y, dy, sizeof(double) * n, hipMemcpyDeviceToHost));
  (void)hipFree(dx); (void)hipFree(dg); (void)hipFree(dy);
  return AGP_OK;
}

int agp_debug_mfma_probe(agp_ctx* c, const double* A, const double* B, double* D) {
  if (!c || !A || !B || !D) return fail(c, AGP_ERR_ARG, "null pointer");
  HIPCHK(c, hipSetDevice(c->device));
  double *dA = nullptr, *dB = nullptr, *dD = nullptr;
  HIPCHK(c, malloc_values(c->poison, (void**)&dA, 64 * 8));
  HIPCHK(c, malloc_values(c->poison, (void**)&dB, 64 * 8));
  HIPCHK(c, malloc_values(c->poison, (void**)&dD, 256 * 8));
  HIPCHK(c, hipMemcpy(dA, A, 64 * 8, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(dB, B, 64 * 8, hipMemcpyHostToDevice));
  launch_mfma_probe(dA, dB, dD);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpy(D, dD, 256 * 8, hipMemcpyDeviceToHost));
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dD);
  return AGP_OK;
}

}  // extern "C"
