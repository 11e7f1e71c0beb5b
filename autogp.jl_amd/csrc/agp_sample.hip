// Host side of posterior predictive sampling: rand(MixtureModel(MvNormal_p, weights), S) of predict_mvn (src/api.jl:497-522) on the
// resident series (agp_predict_sample_batch).  The factorisation is agp_predict_logpdf_batch's joint pass (predict_joint_batch) with a
// zero query right-hand side; per chunk of distinct particles the device read-out k_pred_sample (csrc/agp_sample_kernel.hpp) turns the
// factor into the samples whose component lies in the chunk, before the next chunk overwrites it.
#include "agp_host.hpp"
#include "agp_philox.hpp"

// component of every sample: the caller's, or the inverse CDF of the cumulative weights (particle order, fp64) at the uniform of word 0
// of block (s, 0, 0, 0): the first p with u < cum[p] (a weight-0 particle never raises cum, so it is never first), and the last
// particle of positive weight when rounding leaves u >= cum[P - 1]
void draw_components(int64_t S, int32_t P, const double* w, uint64_t seed, std::vector<int32_t>& comp) {
  std::vector<double> cum((size_t)P);
  double acc = 0.0;
  int32_t last = 0;
  for (int32_t p = 0; p < P; ++p) {
    acc += w[p];
    cum[(size_t)p] = acc;
    if (w[p] > 0.0) last = p;
  }
  for (int64_t s = 0; s < S; ++s) {
    const double u = philox_uniform(philox4x64_10((uint64_t)s, 0, 0, 0, seed, 0).w[0]);
    const auto it = std::upper_bound(cum.begin(), cum.end(), u);
    comp[(size_t)s] = it == cum.end() ? last : (int32_t)(it - cum.begin());
  }
}

extern "C" {

int agp_predict_sample_batch(agp_ctx* c, int64_t n, const double* ts_pred, int64_t m, int32_t P, const int32_t* op_off,
                             const uint8_t* ops, const int32_t* prm_off, const double* prm, const double* noise,
                             const double* noise_pred, const double* mean_train, const double* mean_pred, const double* weights,
                             double y_slope, double y_intercept, int64_t S, uint64_t seed, const int32_t* component, const double* z,
                             double* out_x, int32_t* out_component, int32_t* out_info) {
  return abi_guard(c, [&]() -> int {
    if (!c) return fail(nullptr, AGP_ERR_ARG, "null context");
    if (P <= 0) return fail(c, AGP_ERR_ARG, "P must be >= 1");
    if (n < 0 || m < 0 || S < 0) return fail(c, AGP_ERR_ARG, "negative size");
    if (const int rc = check_resident(c, n)) return rc;
    if (int rc = check_weights(c, P, weights)) return rc;
    if (const int rc = check_y_transform(c, y_slope, y_intercept)) return rc;
    if (m * S >= ((int64_t)1 << 31) || S >= ((int64_t)1 << 31) - 2 * SMP_G) return fail(c, AGP_ERR_ARG, "m * S too large");
    if (component)
      for (int64_t s = 0; s < S; ++s) {
        if (component[s] < 0 || component[s] >= P) return fail(c, AGP_ERR_ARG, "component out of range [0, P)");
        if (!(weights[component[s]] > 0.0)) return fail(c, AGP_ERR_ARG, "component of weight 0");
      }
    if (m == 0 || S == 0) return AGP_OK;
    const Particles pp{P, op_off, ops, prm_off, prm, noise, noise_pred};
    if (!pp.complete() || !ts_pred || !out_x) return fail(c, AGP_ERR_ARG, "null pointer argument");

    std::vector<int32_t> comp((size_t)S);
    if (component) std::copy(component, component + S, comp.begin());
    else draw_components(S, P, weights, seed, comp);

    const int m_pad = round_up(m, NB), nt2 = m_pad / NB;
    const int ldz = round_up(S, 16) + SMP_G;      // (the last group's second sample block reads up to SMP_G - 1 columns past S)
    std::vector<int32_t> order;                // sorted position -> distinct particle (the pass's chunks are runs of it)
    std::vector<int32_t> soff, slist;          // CSR: samples of distinct particle u, ascending: slist[soff[u] .. soff[u + 1])
    std::vector<int32_t> idx;                  // [col (S) | groups (4 per group)]
    std::vector<int> goff;                     // chunk k's groups: [goff[k], goff[k + 1])
    int n_chunk = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;      // (profiling) normals, then one read-out per chunk
    struct EvGuard {
      std::vector<std::pair<hipEvent_t, hipEvent_t>>& v;
      ~EvGuard() { for (auto& e : v) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); } }
    } evg{ev};
    auto mark = [&](hipStream_t st, bool begin) -> hipError_t {
      if (!c->profiling) return hipSuccess;
      hipEvent_t e;
      hipError_t r = hipEventCreate(&e);
      if (r != hipSuccess) return r;
      if (begin) ev.push_back({e, nullptr}); else ev.back().second = e;
      return hipEventRecord(e, st);
    };

    JointHooks h;
    h.plan = [&](int U, const std::vector<int>& rep, const std::vector<int32_t>& ord) {
      order = ord;
      soff.assign((size_t)U + 1, 0);
      for (int64_t s = 0; s < S; ++s) ++soff[(size_t)(rep.empty() ? comp[(size_t)s] : rep[(size_t)comp[(size_t)s]]) + 1];
      for (int u = 0; u < U; ++u) soff[(size_t)u + 1] += soff[(size_t)u];
      slist.resize((size_t)S);
      std::vector<int32_t> fill(soff.begin(), soff.end() - 1);
      for (int64_t s = 0; s < S; ++s) slist[(size_t)fill[(size_t)(rep.empty() ? comp[(size_t)s] : rep[(size_t)comp[(size_t)s]])]++] = (int32_t)s;
      std::lock_guard<std::mutex> g(c->mu);
      c->n_particles_seen += P; c->n_particles_run += U;      // (agp_get_dedup_stats)
      return AGP_OK;
    };
    h.stage = [&](Slot* s, PinnedUploads& up, int chunk) -> int {
      const int U = (int)order.size();
      idx.clear(); idx.reserve((size_t)S + 4 * ((size_t)S / SMP_G + U));
      for (int q = 0; q < U; ++q)
        for (int32_t k = soff[(size_t)order[q]]; k < soff[(size_t)order[q] + 1]; ++k) idx.push_back(slist[(size_t)k]);
      goff.assign(1, 0);
      int j = 0;
      for (int p0 = 0; p0 < U; p0 += chunk) {
        for (int q = p0; q < std::min(U, p0 + chunk); ++q) {
          const int u = order[q], ns = soff[(size_t)u + 1] - soff[(size_t)u];
          for (int g = 0; g < ns; g += SMP_G) {
            idx.insert(idx.end(), {q - p0, j + g, std::min(SMP_G, ns - g), 0});
          }
          j += ns;
        }
        goff.push_back((int)((idx.size() - (size_t)S) / 4));
      }
      HIPCHK(c, s->smp_idx.ensure(sizeof(int32_t) * idx.size()));
      HIPCHK(c, s->smp_z.ensure(sizeof(double) * (size_t)m_pad * ldz));
      HIPCHK(c, s->smp_x.ensure(sizeof(double) * (size_t)m * S));
      up.add(s->smp_idx.p, idx.data(), sizeof(int32_t) * idx.size());
      if (z) {
        HIPCHK(c, s->smp_zin.ensure(sizeof(double) * (size_t)m * S));
        up.add(s->smp_zin.p, z, sizeof(double) * (size_t)m * S);
      }
      return AGP_OK;
    };
    h.chunk = [&](Slot* s, hipStream_t st, const CholArgs& ca, int p0, int Pc) -> int {
      (void)p0; (void)Pc;
      const int32_t* col = s->smp_idx.as<int32_t>();
      if (n_chunk == 0) {
        SampleNormArgs na = {};
        na.Z = s->smp_z.as<double>(); na.m = (int)m; na.m_pad = m_pad; na.ldz = ldz; na.S = (int)S; na.col = col; na.seed = seed;
        na.zin = z ? s->smp_zin.as<double>() : nullptr;
        HIPCHK(c, mark(st, true));
        launch_philox_normals(st, na);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, mark(st, false));
      }
      const int ng = goff[(size_t)n_chunk + 1] - goff[(size_t)n_chunk];
      if (ng > 0) {
        SampleReadArgs ra = {};
        ra.A = ca.A; ra.strideA = ca.strideA; ra.vec = ca.vec; ra.ldv = ca.ldv;
        ra.mu2 = mean_pred ? s->mu2.as<double>() : nullptr;
        ra.Z = s->smp_z.as<double>(); ra.ldz = ldz; ra.col = col; ra.grp = col + S + 4 * (size_t)goff[(size_t)n_chunk];
        ra.nt1 = round_up(n, NB) / NB; ra.m = (int)m;
        ra.zsign = y_slope > 0.0 ? 1.0 : -1.0; ra.slope = y_slope; ra.intercept = y_intercept;
        ra.out = s->smp_x.as<double>();
        HIPCHK(c, mark(st, true));
        launch_pred_sample(st, ng, nt2, ra);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, mark(st, false));
      }
      ++n_chunk;
      return AGP_OK;
    };
    h.done = [&](Slot* s) -> int {
      HIPCHK(c, hipMemcpy(out_x, s->smp_x.p, sizeof(double) * (size_t)m * S, hipMemcpyDeviceToHost));
      if (c->profiling) {
        double t[2] = {0.0, 0.0};
        for (size_t k = 0; k < ev.size(); ++k) {
          float ms = 0.0f;
          HIPCHK(c, hipEventElapsedTime(&ms, ev[k].first, ev[k].second));
          t[k == 0 ? 0 : 1] += ms;
        }
        c->timing[12] = t[0]; c->timing[13] = t[1];
      }
      return AGP_OK;
    };

    std::vector<double> lp((size_t)P);
    std::vector<int32_t> info((size_t)P, 0);
    const int rc = predict_joint_batch(c, {n, ts_pred, m, mean_train, mean_pred}, nullptr, pp, lp.data(), info.data(), &h);
    if (rc) return rc;
    if (out_component) std::copy(comp.begin(), comp.end(), out_component);
    if (out_info) std::copy(info.begin(), info.end(), out_info);
    // a particle without a predictive: the reference throws building its MvNormal — no sample is valid
    if (std::any_of(info.begin(), info.end(), [](int32_t v) { return v != 0; }))
      std::fill(out_x, out_x + (size_t)m * S, std::numeric_limits<double>::quiet_NaN());
    return AGP_OK;
  });
}

}  // extern "C"
