// Stand-alone check of autogp.jl_amd/csrc/agp_particles.hpp (host only: no HIP, no context).  Every expectation is written out.
// Built and run by tests/test_particles_cpu.py with -fsanitize=address,undefined where the runtimes exist.
#include "agp_particles.hpp"

#include <cstring>

static int failures = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) { ++failures; fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); } \
  } while (0)

template <class T> static bool same(const std::vector<T>& a, const std::vector<typename std::vector<T>::value_type>& b) { return a == b; }
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// P = 6:  0 and 3 exact copies;  1 differs from 0 in noise_pred only;  2 differs from 0 in the sign bit of a zero parameter;
// 4 has no parameter;  5 another program
static const int32_t OP_OFF[7] = {0, 2, 4, 6, 8, 9, 12};
static const uint8_t OPS[12] = {3, 0, 3, 0, 3, 0, 3, 0, 1, 3, 4, 6};
static const int32_t PRM_OFF[7] = {0, 2, 4, 6, 8, 8, 11};
static const double PRM[11] = {0.0, 1.5, 0.0, 1.5, -0.0, 1.5, 0.0, 1.5, 2.0, 3.0, 4.0};
static const double NOISE[6] = {0.1, 0.1, 0.1, 0.1, 0.2, 0.3};
static const double NOISE_PRED[6] = {0.5, 0.6, 0.5, 0.5, 0.5, 0.5};
static Particles population(bool with_pred) { return {6, OP_OFF, OPS, PRM_OFF, PRM, NOISE, with_pred ? NOISE_PRED : nullptr}; }

static std::string key_of(std::initializer_list<uint8_t> ops, std::initializer_list<double> prm, double noise, const double* noise_pred) {
  const int32_t lens[2] = {(int32_t)ops.size(), (int32_t)prm.size()};
  std::string k(reinterpret_cast<const char*>(lens), sizeof lens);
  for (uint8_t o : ops) k.push_back((char)o);
  for (double x : prm) k.append(reinterpret_cast<const char*>(&x), sizeof x);
  k.append(reinterpret_cast<const char*>(&noise), sizeof noise);
  if (noise_pred) k.append(reinterpret_cast<const char*>(noise_pred), sizeof *noise_pred);
  return k;
}

static void test_distinct() {
  std::vector<int> rep, uniq;
  std::vector<std::string> keys;
  CHECK(distinct_particles(population(true), rep, uniq, &keys));
  CHECK(same(rep, {0, 1, 2, 0, 3, 4}));
  CHECK(same(uniq, {0, 1, 2, 4, 5}));
  const double p5 = 0.5, p6 = 0.6;
  CHECK(keys.size() == 5);
  if (keys.size() == 5) {
    CHECK(keys[0] == key_of({3, 0}, {0.0, 1.5}, 0.1, &p5));
    CHECK(keys[1] == key_of({3, 0}, {0.0, 1.5}, 0.1, &p6));
    CHECK(keys[2] == key_of({3, 0}, {-0.0, 1.5}, 0.1, &p5));      // bitwise: -0.0 is not 0.0
    CHECK(keys[2] != keys[0]);
    CHECK(keys[3] == key_of({1}, {}, 0.2, &p5));
    CHECK(keys[4] == key_of({3, 4, 6}, {2.0, 3.0, 4.0}, 0.3, &p5));
  }
  // without noise_pred the pair that differs in it alone collapses
  CHECK(distinct_particles(population(false), rep, uniq, &keys));
  CHECK(same(rep, {0, 0, 1, 0, 2, 3}));
  CHECK(same(uniq, {0, 2, 4, 5}));
  CHECK(keys.size() == 4 && keys[0] == key_of({3, 0}, {0.0, 1.5}, 0.1, nullptr) && keys[0] == particle_key(population(false), 3));
}

static void test_malformed() {
  const int32_t neg_first[3] = {-1, 1, 2}, dec_op[3] = {0, 2, 1}, ok_op[3] = {0, 1, 2}, dec_prm[3] = {0, 1, 0}, ok_prm[3] = {0, 0, 0};
  const uint8_t ops[2] = {1, 1};
  const double prm[1] = {0.0}, nz[2] = {0.1, 0.1};
  const Particles bad[3] = {{2, neg_first, ops, ok_prm, prm, nz, nullptr}, {2, dec_op, ops, ok_prm, prm, nz, nullptr},
                            {2, ok_op, ops, dec_prm, prm, nz, nullptr}};
  for (const Particles& pp : bad) {
    std::vector<int> rep{7}, uniq{7};
    std::vector<std::string> keys{"x"};
    CHECK(!offsets_sane(pp));
    CHECK(!distinct_particles(pp, rep, uniq, &keys));
    CHECK(rep.empty() && uniq.empty() && keys.empty());
    const Distinct D(pp, true);      // every particle is its own representative, nothing is indexed
    CHECK(!D.packed() && D.U() == 2 && D.run().op_off == pp.op_off);
  }
  CHECK(offsets_sane({2, ok_op, ops, ok_prm, prm, nz, nullptr}));
}

static void test_pack_view() {
  SubBatch S;
  pack_particles({5, 4, 2}, population(true), S);
  const Particles v = S.view();
  CHECK(v.P == 3 && S.size() == 3);
  CHECK(same(S.op_off, {0, 3, 4, 6}) && same(S.prm_off, {0, 3, 3, 5}));
  CHECK(same(S.ops, {3, 4, 6, 1, 3, 0}));
  CHECK(S.prm.size() == 5 && S.prm[0] == 2.0 && S.prm[1] == 3.0 && S.prm[2] == 4.0 && same_bits(S.prm[3], -0.0) && S.prm[4] == 1.5);
  CHECK(same(S.noise, {0.3, 0.2, 0.1}) && same(S.noise_pred, {0.5, 0.5, 0.5}));
  CHECK(v.noise_pred == S.noise_pred.data() && v.n_ops(1) == 1 && v.n_prm(1) == 0 && v.program(2)[0] == 3 && same_bits(v.params(2)[0], -0.0));
  // no noise_pred from the caller: none in the view
  pack_particles({0}, population(false), S);
  CHECK(S.noise_pred.empty() && S.view().noise_pred == nullptr);
  // an all-empty parameter set still has one element to point at
  pack_particles({4, 4}, population(false), S);
  CHECK(same(S.prm, {0.0}) && same(S.prm_off, {0, 0, 0}) && S.view().prm == S.prm.data() && same(S.ops, {1, 1}));
  S.outputs(true);
  CHECK(S.lp.size() == 2 && S.info.size() == 2 && S.grad.size() == 1 && S.gnoise.size() == 2);
}

static void test_scatter() {
  const Particles pp = population(false);      // rep = {0, 0, 1, 0, 2, 3}
  const Distinct D(pp, true);
  CHECK(D.packed() && D.copies() && D.U() == 4);
  const Particles run = D.run();
  CHECK(run.P == 4 && run.op_off == D.S.op_off.data() && run.noise_pred == nullptr);
  CHECK(same(D.S.prm_off, {0, 2, 4, 4, 7}));
  const double lp[4] = {10.0, 11.0, 12.0, 13.0};
  std::vector<double> out(6, -1.0);
  D.scatter(lp, out.data());
  CHECK(same(out, {10.0, 10.0, 11.0, 10.0, 12.0, 13.0}));
  const int32_t two[8] = {0, 1, 10, 11, 20, 21, 30, 31};
  std::vector<int32_t> out2(12, -1);
  D.scatter(two, out2.data(), 2);
  CHECK(same(out2, {0, 1, 0, 1, 10, 11, 0, 1, 20, 21, 30, 31}));
  D.scatter(lp, static_cast<double*>(nullptr));      // an output the caller did not ask for
  const double grad[7] = {1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0};
  std::vector<double> g(11, -1.0);
  D.scatter_csr(grad, g.data());
  CHECK(same(g, {1.0, 2.0, 1.0, 2.0, 3.0, 4.0, 1.0, 2.0, 5.0, 6.0, 7.0}));
  // nothing to pack: the caller's own pointers, no copy
  const Particles four{4, OP_OFF + 2, OPS, PRM_OFF + 2, PRM, NOISE + 2, nullptr};      // particles 2 .. 5: no copies
  const Distinct N(four, true);
  CHECK(!N.packed() && !N.copies() && N.U() == 4 && N.S.size() == 0);
  CHECK(N.run().op_off == four.op_off && N.run().ops == OPS && N.run().prm_off == four.prm_off && N.run().prm == PRM && N.run().noise == four.noise);
  const Distinct off(pp, false);
  CHECK(!off.packed() && off.U() == 6 && off.rep.empty() && off.run().op_off == OP_OFF && off.run().prm == PRM && off.rep_of(3) == 3);
  std::vector<double> id(6, -1.0);
  const double six[6] = {0.0, 1.0, 2.0, 3.0, 4.0, 5.0};
  off.scatter(six, id.data());
  CHECK(same(id, {0.0, 1.0, 2.0, 3.0, 4.0, 5.0}));
  // an entry whose pass reads the packed arrays whatever the population
  const Distinct A(four, false, Distinct::Pack::always, true);
  CHECK(A.packed() && !A.copies() && A.U() == 4 && same(A.uniq, {0, 1, 2, 3}) && A.run().op_off == A.S.op_off.data() && A.keys.empty());
  const Distinct K(pp, true, Distinct::Pack::always, true);
  CHECK(K.packed() && K.U() == 4 && K.keys.size() == 4 && K.keys[3] == particle_key(pp, 5));
}

static void test_composite() {
  // two particles of two components each; the first particle alone for M = 1 (its first component)
  const int32_t oo[5] = {0, 1, 4, 5, 6}, po[5] = {0, 1, 4, 5, 5};
  const uint8_t ops[6] = {3, 1, 5, 7, 4, 1};
  const double prm[5] = {0.5, 1.0, 2.0, 3.0, 9.0};
  const Particles comp{2, oo, ops, po, prm, nullptr, nullptr};
  std::vector<uint8_t> cops; std::vector<double> cprm;
  std::string err;
  CHECK(append_composite(comp, 0, 1, AGP_MAX_OPS, cops, cprm, err) == AGP_OK);
  CHECK(same(cops, {3, 10, 7}) && same(cprm, {0.5, 1.0}));
  cops.clear(); cprm.clear();
  CHECK(append_composite(comp, 0, 2, AGP_MAX_OPS, cops, cprm, err) == AGP_OK);
  CHECK(same(cops, {3, 10, 7, 1, 5, 7, 10, 7, 6}) && same(cprm, {0.5, 1.0, 1.0, 2.0, 3.0, 2.0}));
  // the second particle's composite is appended behind the first's
  CHECK(append_composite(comp, 2, 2, AGP_MAX_OPS, cops, cprm, err) == AGP_OK);
  CHECK(cops.size() == 16 && same(std::vector<uint8_t>(cops.begin() + 9, cops.end()), {4, 10, 7, 1, 10, 7, 6}));
  CHECK(same(std::vector<double>(cprm.begin() + 6, cprm.end()), {9.0, 1.0, 2.0}));
  // refusals
  const uint8_t bad_ops[6] = {3, 1, 9, 7, 4, 1};
  cops.clear(); cprm.clear();
  CHECK(append_composite({2, oo, bad_ops, po, prm, nullptr, nullptr}, 0, 2, AGP_MAX_OPS, cops, cprm, err) == AGP_ERR_PROGRAM);
  CHECK(err == "unknown opcode");
  const int32_t long_oo[2] = {0, AGP_MAX_OPS - 1}, long_po[2] = {0, 0};      // + SEL + TIMES = AGP_MAX_OPS + 1 nodes
  const std::vector<uint8_t> long_ops((size_t)AGP_MAX_OPS - 1, 6);
  cops.clear(); cprm.clear();
  CHECK(append_composite({1, long_oo, long_ops.data(), long_po, prm, nullptr, nullptr}, 0, 1, AGP_MAX_OPS, cops, cprm, err) == AGP_ERR_PROGRAM);
  CHECK(err == "composite program longer than AGP_MAX_OPS (255) nodes" && cops.size() == (size_t)AGP_MAX_OPS + 1);
  const int32_t fit_oo[2] = {0, AGP_MAX_OPS - 2};
  cops.clear(); cprm.clear();
  CHECK(append_composite({1, fit_oo, long_ops.data(), long_po, prm, nullptr, nullptr}, 0, 1, AGP_MAX_OPS, cops, cprm, err) == AGP_OK);
  const int32_t dec_oo[3] = {0, 2, 1};
  cops.clear(); cprm.clear();
  CHECK(append_composite({2, dec_oo, ops, po, prm, nullptr, nullptr}, 0, 2, AGP_MAX_OPS, cops, cprm, err) == AGP_ERR_ARG);
  CHECK(err == "malformed offsets of component 2");
}

int main() {
  test_distinct();
  test_malformed();
  test_pack_view();
  test_scatter();
  test_composite();
  if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  puts("particles_test: ok");
  return 0;
}
