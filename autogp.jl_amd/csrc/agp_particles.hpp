// A population of particles as the host code passes it around: one non-owning view instead of seven loose pointers, the owning
// sub-batch cut out of one, and what every host entry does with a resampled population — find the distinct particles, run them
// once, hand every copy its representative's results.  Host only, plain C++: no HIP, no context (tests/native/particles_test.cpp
// builds it alone).
#pragma once
#include "../../include/autogp_hip.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>

// CSR programs and parameters of P particles (particle p: ops[op_off[p] .. op_off[p + 1]), prm likewise) and their noises.
// noise_pred may be null (predictive entries: each particle's own noise).
struct Particles {
  int P;
  const int32_t* op_off; const uint8_t* ops; const int32_t* prm_off; const double* prm;
  const double* noise; const double* noise_pred;
  bool complete() const { return op_off && ops && prm_off && prm && noise; }      // (what the entries' null-pointer checks ask)
  const uint8_t* program(int p) const { return ops + op_off[p]; }
  int n_ops(int p) const { return op_off[p + 1] - op_off[p]; }
  const double* params(int p) const { return prm + prm_off[p]; }
  int n_prm(int p) const { return prm_off[p + 1] - prm_off[p]; }
};

// offsets that are non-negative and non-decreasing (everything that indexes with them asks first)
inline bool offsets_sane(const Particles& pp) {
  for (int p = 0; p < pp.P; ++p)
    if (pp.op_off[p + 1] < pp.op_off[p] || pp.prm_off[p + 1] < pp.prm_off[p] || pp.op_off[p] < 0 || pp.prm_off[p] < 0) return false;
  return true;
}

// key of a particle in the factor store: the bits of (program, parameters, noise)
inline std::string particle_key(const uint8_t* ops, int no, const double* prm, int np, double noise) {
  std::string key;
  const int32_t lens[2] = {no, np};
  key.assign(reinterpret_cast<const char*>(lens), sizeof lens);
  key.append(reinterpret_cast<const char*>(ops), (size_t)no);
  key.append(reinterpret_cast<const char*>(prm), sizeof(double) * (size_t)np);
  key.append(reinterpret_cast<const char*>(&noise), sizeof(double));
  return key;
}
inline std::string particle_key(const Particles& pp, int p) {
  return particle_key(pp.program(p), pp.n_ops(p), pp.params(p), pp.n_prm(p), pp.noise[p]);
}

// Distinct particles of a batch (a resampled population holds copies of its survivors), keyed by particle_key (+ the bits of
// noise_pred[p] when given): uniq = the first particle of each, in the caller's order; rep[p] = the position in uniq of p's;
// keys (optional) = uniq's keys.  False, with everything empty, on offsets that are negative or decreasing: the caller decides.
inline bool distinct_particles(const Particles& pp, std::vector<int>& rep, std::vector<int>& uniq, std::vector<std::string>* keys = nullptr) {
  rep.clear(); uniq.clear();
  if (keys) keys->clear();
  if (!offsets_sane(pp)) return false;
  std::unordered_map<std::string, int> seen;
  seen.reserve((size_t)pp.P * 2);
  rep.resize((size_t)pp.P);
  for (int p = 0; p < pp.P; ++p) {
    std::string key = particle_key(pp, p);
    if (pp.noise_pred) key.append(reinterpret_cast<const char*>(pp.noise_pred + p), sizeof(double));
    const auto it = seen.try_emplace(std::move(key), (int)uniq.size());
    rep[(size_t)p] = it.first->second;
    if (it.second) { uniq.push_back(p); if (keys) keys->push_back(it.first->first); }
  }
  return true;
}

// Some particles of a caller's batch packed into a batch of their own, in the order of the index list: offsets, concatenated
// programs / parameters (an empty parameter array holds one 0.0: never a null pointer), noises; noise_pred when the caller passes
// one.  lp / info / grad / gnoise: the sub-batch's outputs, sized by outputs().
struct SubBatch {
  std::vector<int32_t> op_off, prm_off;
  std::vector<uint8_t> ops;
  std::vector<double> prm, noise, noise_pred;
  std::vector<double> lp, grad, gnoise;
  std::vector<int32_t> info;
  int size() const { return (int)noise.size(); }
  void outputs(bool with_grad) {
    lp.assign(noise.size(), 0.0); info.assign(noise.size(), 0);
    if (with_grad) { grad.assign(prm.size(), 0.0); gnoise.assign(noise.size(), 0.0); }
  }
  Particles view() const {
    return {size(), op_off.data(), ops.data(), prm_off.data(), prm.data(), noise.data(), noise_pred.empty() ? nullptr : noise_pred.data()};
  }
};

inline void pack_particles(const std::vector<int>& ix, const Particles& pp, SubBatch& S) {
  const size_t B = ix.size();
  S.op_off.assign(B + 1, 0); S.prm_off.assign(B + 1, 0); S.ops.clear(); S.prm.clear();
  S.noise.resize(B); S.noise_pred.resize(pp.noise_pred ? B : 0);
  for (size_t b = 0; b < B; ++b) {
    const int p = ix[b];
    S.ops.insert(S.ops.end(), pp.program(p), pp.program(p) + pp.n_ops(p));
    S.prm.insert(S.prm.end(), pp.params(p), pp.params(p) + pp.n_prm(p));
    S.op_off[b + 1] = (int32_t)S.ops.size(); S.prm_off[b + 1] = (int32_t)S.prm.size();
    S.noise[b] = pp.noise[p];
    if (pp.noise_pred) S.noise_pred[b] = pp.noise_pred[p];
  }
  if (S.prm.empty()) S.prm.push_back(0.0);
}

// The distinct particles of a caller's population, ready to run once each.  `dedup` off (the context's switch) or malformed offsets:
// every particle is its own representative.  Without copies nothing is packed and run() is the caller's own view — no copy of the
// population is made — unless the entry asks for Pack::always (its pass then reads the packed arrays whatever the population).
struct Distinct {
  enum class Pack { when_copies, always };
  std::vector<int> rep, uniq;           // (distinct_particles; both empty: nothing was deduplicated)
  std::vector<std::string> keys;        // uniq's keys, on request
  SubBatch S;
  Distinct(const Particles& pp, bool dedup, Pack pack = Pack::when_copies, bool want_keys = false) : caller_(pp) {
    if (dedup) (void)distinct_particles(pp, rep, uniq, want_keys ? &keys : nullptr);
    packed_ = pack == Pack::always || copies();
    if (!packed_) return;
    if (uniq.empty()) { uniq.resize((size_t)pp.P); for (int p = 0; p < pp.P; ++p) uniq[(size_t)p] = p; }
    pack_particles(uniq, pp, S);
  }
  int U() const { return uniq.empty() ? caller_.P : (int)uniq.size(); }
  bool copies() const { return U() < caller_.P; }
  bool packed() const { return packed_; }
  Particles run() const { return packed_ ? S.view() : caller_; }
  int rep_of(int p) const { return rep.empty() ? p : rep[(size_t)p]; }
  // fixed-stride outputs: caller particle p receives its representative's `stride` values (a null side: nothing to do)
  template <class T> void scatter(const T* src, T* dst, size_t stride = 1) const {
    if (!src || !dst) return;
    for (int p = 0; p < caller_.P; ++p) std::copy_n(src + (size_t)rep_of(p) * stride, stride, dst + (size_t)p * stride);
  }
  // CSR outputs (gradients): src laid out by the run's prm_off, dst by the caller's
  void scatter_csr(const double* src, double* dst) const {
    const Particles r = run();
    for (int p = 0; p < caller_.P; ++p) {
      const int u = rep_of(p);
      std::copy(src + r.prm_off[u], src + r.prm_off[u + 1], dst + caller_.prm_off[p]);
    }
  }
 private:
  Particles caller_;
  bool packed_ = false;
};

// The composite program of a sum of GPs, K_1 SEL_1 *  K_2 SEL_2 * +  ...  K_M SEL_M * +, appended to cops / cprm from the M
// components [first, first + M) of `components` (one CSR entry each).  The operator codes are the C ABI's, the selector leaf is the
// engine's OP_SEL (agp_host.hpp checks both against agp_common.hpp).  max_ops: the length is checked after every component.
// Returns AGP_OK, or the error code with the reason in err.
constexpr uint8_t COMPOSITE_OP_PLUS = 6, COMPOSITE_OP_TIMES = 7, COMPOSITE_OP_LAST = 8, COMPOSITE_OP_SEL = 10;
inline int append_composite(const Particles& components, int64_t first, int M, int max_ops, std::vector<uint8_t>& cops,
                            std::vector<double>& cprm, std::string& err) {
  const int32_t* oo = components.op_off; const int32_t* po = components.prm_off;
  const size_t o0 = cops.size();
  char buf[128];
  for (int i = 0; i < M; ++i) {
    const int64_t k = first + i;
    if (oo[k] < 0 || po[k] < 0 || oo[k + 1] < oo[k] || po[k + 1] < po[k]) {
      snprintf(buf, sizeof buf, "malformed offsets of component %d", i + 1);
      err = buf;
      return AGP_ERR_ARG;
    }
    for (int q = oo[k]; q < oo[k + 1]; ++q) {
      if (components.ops[q] > COMPOSITE_OP_LAST) { err = "unknown opcode"; return AGP_ERR_PROGRAM; }
      cops.push_back(components.ops[q]);
    }
    cprm.insert(cprm.end(), components.prm + po[k], components.prm + po[k + 1]);
    cops.push_back(COMPOSITE_OP_SEL); cprm.push_back((double)(i + 1));
    cops.push_back(COMPOSITE_OP_TIMES);
    if (i > 0) cops.push_back(COMPOSITE_OP_PLUS);
    if (cops.size() - o0 > (size_t)max_ops) {
      snprintf(buf, sizeof buf, "composite program longer than AGP_MAX_OPS (%d) nodes", max_ops);
      err = buf;
      return AGP_ERR_PROGRAM;
    }
  }
  return AGP_OK;
}
