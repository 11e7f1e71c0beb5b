// The reverse-mode pass of the gradient contractions over E matrix elements in lockstep, with its tape and accumulator types: shared
// by the tiled sweep's k_grad_contract (agp_grad_kernel.hpp) and the short-series kernel k_series_logpdf_grad (agp_series_kernel.hpp).
#pragma once
#include "agp_common.hpp"
#include "agp_args.hpp"
#include "agp_math.hpp"

namespace agp {

// ---- reverse-mode pass over E elements in lockstep ----------------------------------------------
// One private-memory slot per node and element: it holds the node's VALUE after the forward pass and is
// overwritten by the node's ADJOINT when its parent is visited in the backward pass (a binary node only
// needs its children's values, never its own; a stationary leaf is handed adjoint x value so that it does not
// evaluate its exponential again).  gacc: per parameter slot accumulator.
// The E elements share one walk over the program, so their memory latencies overlap.
// Node values / adjoints of the tape variant of the contraction.  RegTape: a private array (dynamic node indices put it in
// scratch memory; any tree size).  LdsTape: one column of a [node][element][thread] array in LDS (trees of <= LDS_TAPE_NODES
// nodes): the backward sweep is a chain of dependent tape round trips per node, ~60 cycles each in LDS instead of a
// global-memory round trip (measured: ~6 ms per tree node and 512-particle sweep at n=2048 with the scratch tape).
template <int MAXS, int E>
struct RegTape {
  double v[MAXS][E];
  __device__ __forceinline__ double get(int i, int e) const { return v[i][e]; }
  __device__ __forceinline__ void set(int i, int e, double x) { v[i][e] = x; }
};
template <int E>
struct LdsTape {
  double* base;      // this thread's column: element (i, e) at base[(i * E + e) * 256]
  __device__ __forceinline__ double get(int i, int e) const { return base[(i * E + e) * 256]; }
  __device__ __forceinline__ void set(int i, int e, double x) { base[(i * E + e) * 256] = x; }
};

// Per-parameter gradient accumulators of one thread: an array indexed by parameter offset (private memory).  (Register
// accumulators selected by the leaf's ordinal were measured for the LDS-tape variant: no gain — the accumulator updates are
// not on the critical path, the tape round trips were.)
template <int N>
struct ScratchAcc {
  double (&g)[N];
  __device__ __forceinline__ void leaf(int po, int, double g0, double g1, double g2) { g[po] += g0; g[po + 1] += g1; g[po + 2] += g2; }
  __device__ __forceinline__ void cp(int po, int, double g0, double g1) { g[po] += g0; g[po + 1] += g1; }
};
// CSIG: the per-point tables are followed by their complements — table h.n_cp + c holds 1 - sigma of ChangePoint c, formed as
// (1 - tanh) / 2 from the same tanh (exact where sigma is near 1) — and 1 - sigma is read there instead of being subtracted from the
// rounded sigma, which keeps only ulp(1) / (1 - sigma) of it: a ChangePoint at the prior's scale 1e-3 has every point but its nearest
// at |loc - t| / scale > 10, and the derivative by the scale consists of such terms alone (k_series_logpdf_grad; the tiled sweep's
// kernels keep the subtraction and their bits).
template <int MAXS, int E, bool CSIG = false, class TapeT, class AccT>
__device__ __forceinline__ void grad_elements(const GProgHdr& h, const uint8_t* ops, const uint8_t* lc, const uint8_t* rc,
                                              const uint8_t* mv, const int32_t* poff, const double* prm, const double* sig,
                                              const int (&ri)[E], const int (&ci)[E], const double (&ta)[E],
                                              const double (&tb)[E], const double (&wgt)[E],
                                              const double (&lt)[E], bool use_tab,
                                              TapeT& tape, AccT& acc) {
  const double PI = 3.14159265358979323846;
  // ---------------- forward: node values ----------------
  int cpi = 0, nl = 0, nb = 0;      // ChangePoint tables / leaves / binary nodes seen so far (wave-uniform)
  for (int ip = 0; ip < h.n_ops; ++ip) {
    const int o = __builtin_amdgcn_readfirstlane((int)ops[ip]);
    const double* q = prm + poff[ip];
    const double q0 = q[0], q1 = q[1], q2 = q[2];
    const int il = lc[ip], ir = rc[ip];
    const double lgl = (use_tab && o == OP_GE) ? fm::log_f(q0) : 0.0;      // once per node visit, not per element
    if (o <= OP_PER) ++nl; else ++nb;
    // (the opcode dispatch stays OUTSIDE the element loops: each branch is one basic block in which the E independent
    // evaluation chains interleave)
    double v[E];
    if (o == OP_WN) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = (ta[e] == tb[e]) ? q0 : 0.0;
    } else if (o == OP_CONST) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = q0;
    } else if (o == OP_LIN) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = q1 + q2 * ((ta[e] - q0) * (tb[e] - q0));
    } else if (o == OP_SE) {
      const double c2 = -0.5 / (q0 * q0);
#pragma unroll
      for (int e = 0; e < E; ++e) { const double d = ta[e] - tb[e]; v[e] = q1 * fm::exp_f((d * d) * c2); }
    } else if (o == OP_GE) {
      // with the data set's log|dt| table (lt): (|dt|/l)^g = exp(g (log|dt| - log l)), no per-element log
      if (use_tab) {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = q2 * fm::exp_f(-fm::exp_f(q1 * (lt[e] - lgl)));
      } else {
        const double rl = 1.0 / q0;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = q2 * fm::exp_f(-fm::pow_f(fabs(ta[e] - tb[e]) * rl, q1));
      }
    } else if (o == OP_PER) {
      const double wq = PI / q1, c2 = -2.0 / (q0 * q0);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = q2 * fm::exp_f(c2 * fm::sin2_f(wq * fabs(ta[e] - tb[e])));
    } else if (o == OP_PLUS) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = tape.get(il, e) + tape.get(ir, e);
    } else if (o == OP_TIMES) {
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = tape.get(il, e) * tape.get(ir, e);
    } else {   // OP_CP (children by true left / right index)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const double sa = sig[cpi * 256 + ri[e]], sb = sig[cpi * 256 + ci[e]];
        if constexpr (CSIG) {
          const double ya = sig[(h.n_cp + cpi) * 256 + ri[e]], yb = sig[(h.n_cp + cpi) * 256 + ci[e]];
          v[e] = (sa * sb) * tape.get(il, e) + (ya * yb) * tape.get(ir, e);
        } else {
          v[e] = (sa * sb) * tape.get(il, e) + ((1.0 - sa) * (1.0 - sb)) * tape.get(ir, e);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) tape.set(ip, e, v[e]);
    if (o == OP_CP) ++cpi;
  }
  // ---------------- backward: adjoints replace values top-down ----------------
  // A stationary leaf with a non-zero amplitude (mv[node] = 1) receives adjoint * VALUE instead of the
  // adjoint: its derivatives are that product times a factor free of the exponential
  // (SE: d/d amp = s/amp, d/d l = s d^2/l^3, ...), so the backward pass re-evaluates no exp.
  {
    const int root = h.n_ops - 1;
    const bool m = __builtin_amdgcn_readfirstlane((int)mv[root]) != 0;
#pragma unroll
    for (int e = 0; e < E; ++e) tape.set(root, e, m ? wgt[e] * tape.get(root, e) : wgt[e]);
  }
  for (int ip = h.n_ops - 1; ip >= 0; --ip) {
    const int o = __builtin_amdgcn_readfirstlane((int)ops[ip]);
    const int po = poff[ip];
    const double* q = prm + po;
    const double q0 = q[0], q1 = q[1], q2 = q[2];
    const int il = lc[ip], ir = rc[ip];
    const bool m = __builtin_amdgcn_readfirstlane((int)mv[ip]) != 0;
    if (o == OP_CP) --cpi;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;
    if (o <= OP_PER) --nl; else --nb;          // forward ordinal of this node among the leaves / binary nodes
    if (o <= OP_PER) {
      if (o == OP_WN) {
#pragma unroll
        for (int e = 0; e < E; ++e) g0 += (ta[e] == tb[e]) ? tape.get(ip, e) : 0.0;
      } else if (o == OP_CONST) {
#pragma unroll
        for (int e = 0; e < E; ++e) g0 += tape.get(ip, e);
      } else if (o == OP_LIN) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double ad = tape.get(ip, e);
          g0 += ad * (-q2 * (ta[e] + tb[e] - 2.0 * q0));
          g1 += ad;
          g2 += ad * ((ta[e] - q0) * (tb[e] - q0));
        }
      } else if (o == OP_SE) {
        if (m) {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const double sv = tape.get(ip, e), d = ta[e] - tb[e];
            g0 += sv * (d * d);
            g1 += sv;
          }
          g0 *= 1.0 / (q0 * q0 * q0);
          g1 *= 1.0 / q1;
        } else {
#pragma unroll
          for (int e = 0; e < E; ++e) {
            const double ad = tape.get(ip, e), d = ta[e] - tb[e], d2 = d * d;
            const double ex = fm::exp_f(-0.5 * d2 / (q0 * q0));
            g0 += ad * q1 * ex * d2 / (q0 * q0 * q0);
            g1 += ad * ex;
          }
        }
      } else if (o == OP_GE) {
        const double rl = 1.0 / q0;
        const double lgl = use_tab ? fm::log_f(q0) : 0.0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          double lu, ug;
          if (use_tab) {
            lu = lt[e] - lgl;                                        // dt = 0: table sentinel, exp -> 0 exactly, 0 * lu = -0
            ug = fm::exp_f(q1 * lu);
          } else {
            const double u = fabs(ta[e] - tb[e]) * rl;
            lu = fm::log_f(u > 0.0 ? u : 1.0);                       // u^g ln u -> 0 at u = 0
            ug = u > 0.0 ? fm::exp_f(q1 * lu) : 0.0;
          }
          const double sv = m ? tape.get(ip, e) : tape.get(ip, e) * fm::exp_f(-ug);   // adjoint * amp * exp  |  adjoint * exp
          g0 += sv * ug;
          g1 -= sv * (ug * lu);
          g2 += sv;
        }
        if (m) { g0 *= q1 * rl; g2 *= 1.0 / q2; }
        else { g0 *= q2 * q1 * rl; g1 *= q2; }
      } else {   // OP_PER
        const double l2 = q0 * q0, wq = PI / q1;
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double dd = fabs(ta[e] - tb[e]);
          double sn, cs;
          fm::sincos_pi_f(wq * dd, &sn, &cs);
          const double sv = m ? tape.get(ip, e) : tape.get(ip, e) * fm::exp_f(-2.0 * sn * sn / l2);
          g0 += sv * (sn * sn);
          g1 += sv * (sn * cs * dd);
          g2 += sv;
        }
        const double f0 = 4.0 / (l2 * q0), f1 = 4.0 * PI / (l2 * q1 * q1);
        if (m) { g0 *= f0; g1 *= f1; g2 *= 1.0 / q2; }
        else { g0 *= q2 * f0; g1 *= q2 * f1; }
      }
      acc.leaf(po, nl, g0, g1, g2);
    } else {
      const bool ml = __builtin_amdgcn_readfirstlane((int)mv[il]) != 0, mr = __builtin_amdgcn_readfirstlane((int)mv[ir]) != 0;
      if (o == OP_PLUS) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double ad = tape.get(ip, e);
          tape.set(il, e, ml ? ad * tape.get(il, e) : ad);
          tape.set(ir, e, mr ? ad * tape.get(ir, e) : ad);
        }
      } else if (o == OP_TIMES) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double ad = tape.get(ip, e), kl = tape.get(il, e), kr = tape.get(ir, e);
          const double al_ = ad * kr, ar_ = ad * kl;
          tape.set(il, e, ml ? al_ * kl : al_);
          tape.set(ir, e, mr ? ar_ * kr : ar_);
        }
      } else {   // OP_CP: q = {location, scale}
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const double ad = tape.get(ip, e);
          const double x1 = sig[cpi * 256 + ri[e]], x2 = sig[cpi * 256 + ci[e]];
          const double kl = tape.get(il, e), kr = tape.get(ir, e);
          if constexpr (CSIG) {
            const double y1 = sig[(h.n_cp + cpi) * 256 + ri[e]], y2 = sig[(h.n_cp + cpi) * 256 + ci[e]];      // 1 - sigma
            const double al_ = ad * (x1 * x2), ar_ = ad * (y1 * y2);
            tape.set(il, e, ml ? al_ * kl : al_);
            tape.set(ir, e, mr ? ar_ * kr : ar_);
            const double da = 2.0 * x1 * y1 / q1, db = 2.0 * x2 * y2 / q1;
            g0 += ad * ((da * x2 + x1 * db) * kl - (da * y2 + y1 * db) * kr);
            const double das = -da * (q0 - ta[e]) / q1, dbs = -db * (q0 - tb[e]) / q1;
            g1 += ad * ((das * x2 + x1 * dbs) * kl - (das * y2 + y1 * dbs) * kr);
          } else {
            const double al_ = ad * (x1 * x2), ar_ = ad * ((1.0 - x1) * (1.0 - x2));
            tape.set(il, e, ml ? al_ * kl : al_);
            tape.set(ir, e, mr ? ar_ * kr : ar_);
            // d sigma / d loc = 2 sigma (1 - sigma) / scale;  d sigma / d scale = -(loc - t)/scale * that
            const double da = 2.0 * x1 * (1.0 - x1) / q1, db = 2.0 * x2 * (1.0 - x2) / q1;
            g0 += ad * ((da * x2 + x1 * db) * kl - (da * (1.0 - x2) + (1.0 - x1) * db) * kr);
            const double das = -da * (q0 - ta[e]) / q1, dbs = -db * (q0 - tb[e]) / q1;
            g1 += ad * ((das * x2 + x1 * dbs) * kl - (das * (1.0 - x2) + (1.0 - x1) * dbs) * kr);
          }
        }
        acc.cp(po, nb, g0, g1);
      }
    }
  }
}

}  // namespace agp
