// Argument structs of the kernels and the LDS / table constants the host sizes its launches with: plain data, shared by the
// kernel translation units (agp_kernels.hip, agp_kernels_grad.hip) and the host side (agp_launch.hpp).
#pragma once
#include "agp_common.hpp"

namespace agp {

// COMPACT lag tables — calendar lattices too long for a table over their lags (2048 month starts span 62 304 days; the reference's
// dates arrive through datetime2unix + the min-max transform, src/api.jl:49-51,98-101).  In time order the lattice indices g_i of
// such a series grow almost evenly: all pairs (i, i + od) have lattice lags within base[od] .. base[od] + W - 1 (month starts: W <= 5),
// so a stationary subtree's table needs only W entries per ordinal difference — entry W od + (lag - base[od]) — instead of one per
// lattice lag.  A point's key packs (ordinal << CLT_SHIFT) | g; an element reads table[(|dkey| & CLT_MASK) + B[|dkey| >> CLT_SHIFT]]
// with B[od] = W od - base[od].  W = 0 in the struct: whole tables in LDS (sweeps in the caller's order, W n <= 4096 entries);
// W > 0: sorted sweep, a tile copies the window of its 256 ordinal differences.
constexpr int CLT_SHIFT = 19, CLT_MASK = (1 << CLT_SHIFT) - 1;
struct CltArgs {
  const int32_t* B = nullptr;   // [n_pad + 256] W od - base[od]; null: not a compact sweep
  int W = 0;                    // entries per ordinal difference on a sorted sweep (per-tile windows), 0: whole tables
  int nB = 0;                   // entries of B a tile stages in LDS (even)
  int gstride = 0;              // doubles per table in global memory
};

struct CovArgs {
  const double* tt;      // time points in padded joint layout, length nt*NB
  int n1;                // valid training points  [0, n1)
  int n1_pad;            // start of the prediction segment (multiple of NB)
  int m2;                // valid prediction points [n1_pad, n1_pad+m2)
  int nt;                // tiles per dimension
  const ProgHdr* hdr;    // [P]
  const uint8_t* ops;
  const double* prm;
  const double* noise;   // [P] added on the diagonal of the training block
  double* A;             // packed tiles, per-particle stride strideA
  long long strideA;
  int P;
  int p_off;             // first particle (blockIdx.y is relative to it)
  const uint8_t* code;   // per joint point: 0 observable, i latent of component i (infer_gp_sum); null = all 0
  const double* logdt;   // packed lower tiles of log|t_i - t_j| over the resident data (programs with flags bit 0)
  const int* slot;       // extension sweeps (see CholArgs): storage index per particle, first tile row to (re)build
  const int* i0;
  int skip_pred_offdiag; // prediction without a covariance request: off-diagonal tiles of the K22 block are never read
  int pred_only;         // 1: only the tiles of the prediction block (both indices past the training rows)
  const double* lagtab;  // lag tables of the sweep's OP_LAG_* leaves (k_lag_tables): [table][block lag 0..nt-1][256]
  const int32_t* lagr;   // RANK lag tables (regular grid, points in the caller's order; null: sorted sweep): rank of every resident
  int lag_stride;        //   point in the sorted series; a leaf's table then holds all lag_stride lags 0 .. n_max-1 (see cov_prologue)
  int csplit;            // 4: a tile is shared by four workgroups (grid.z; 32 columns each) — launches of a few large trees,
                         // whose length is ONE workgroup's walk over its tile (launch_cov); otherwise one workgroup per tile
  CltArgs clt;           // compact tables (lagr then holds the points' keys)
  const double* noise_q; // [P] added on the diagonal of the prediction block (agp_predict_logpdf_batch); null everywhere else
};

struct LagArgs {
  const double* tt;        // sorted time points
  const LagTabHdr* thdr;   // [n_tables]
  const uint8_t* tops;
  const double* tprm;
  double* tab;             // [table][nt][256]; full: [table][stride]
  int nt, n_tables;
  int full, stride;        // full = 1: rank tables — grid.x = stride / 256 blocks of lags 256 bl + tid, 0 .. stride-1
};
// structured value sweep (agp_toep_kernel.hpp)
struct ToepArgs {
  const double* xs;          // observations in SORTED order
  int n, P;
  const ProgHdr* hdr;        // programs compiled for a lag sweep: OP_LAG / OP_LIN leaves under OP_PLUS
  const uint8_t* ops;
  const double* prm;
  const double* noise;       // [P]
  const double* lagtab;      // rank-table layout: table t at lagtab + t * lag_stride, lags 0 .. n-1
  int lag_stride;
  double grid_h, grid_mid, tref;
  double* out_lp;            // [P] (sorted particle order)
  int32_t* out_info;         // [P] 0, or 1: refused (the host repeats the particle on the dense path)
  int rank0;                 // rank of the sweep's first point in time (xs already points there; t - t_ref = (rank0 + j - grid_mid) h)
  // gradient sweeps (STORE instantiations / k_toep_back): the columns of L, packed (column k at k n - k (k - 1) / 2, rows k .. n-1),
  // the forward-solved right-hand sides L^-1 [x, e_first, 1, t - t_ref] and the solutions T^-1 [...] (sorted coordinates)
  double* Lcols; long long Lstride;
  double* fwd;               // [P][4][ldv]
  double* sol;               // [P][4][ldv]
  int ldv;
  // predictive sweeps (JOINT instantiation): size of the joint grid (n training points + the future points that follow them), and
  // per future point j: L21 L11^-1 [x, 1, t - t_ref] (rows 0..2) and the Schur complement's diagonal (row 3)
  int nj;
  double* pacc; int pstride;      // [P][4][pstride]
};

struct CholArgs {
  double* A;            // packed tiles
  long long strideA;    // doubles per particle
  double* W;            // [P][NSB][256] inverses of the current diagonal tile's 16x16 blocks
  double* vec;          // [P][ldv]: x on entry, alpha (factored part) / -(V^T alpha) (Schur part) on exit
  int ldv;
  double* partial;      // [P][nt][2]: {log det, alpha'alpha} per block column
  int* info;            // [P]
  int P;
  int nt;               // tile rows of the (joint) matrix
  int k;                // factor mode: block column; Schur mode: unused
  int nt1;              // Schur mode: number of factored block columns
  int tiles;            // factor mode: tiles per particle in this launch (nt-k, or 1 for k = 0)
  int t0;               // sub-diagonal-only launches (DM = 2): the first of them is tile (k + t0, k)
  // fused covariance evaluation (DCOV > 0): the tile is computed from the particle's program
  const double* tt;     // time points, padded joint layout
  int n1, n1_pad, m2;
  const ProgHdr* hdr;
  const uint8_t* ops;
  const double* prm;
  const double* noise;
  const uint8_t* code;  // per-point component codes (infer_gp_sum) or null
  const double* logdt;  // log|dt| table of the resident data (see CovArgs)
  int n_fused;          // particles [0, n_fused) evaluate their tiles; the rest have them prebuilt in A
  int* ready;           // [P] block columns whose L(k,k) is published (in-kernel solve); zeroed per sweep
  int wsteps;           // 1: W holds the current step's inverses only; nt: W keeps every step (gradient path)
  int rl;               // factor mode, right-looking schedule: the tile already holds C(k,k) (no left-looking sum)
  int j0;               // Schur mode: the sum runs over block columns [j0, nt1) (right-looking: one column)
  // Block-extension sweeps over the resident factor store (agp_logpdf_batch_extend): particle p's storage (A, W, vec,
  // partial, info, ready) is slot[p] instead of p, and tile rows below i0[p] already hold its factor from an earlier
  // sweep on a shorter prefix of the data — their workgroups leave at once.  Both null in ordinary sweeps.
  const int* slot;
  const int* i0;
  int ntp;              // row stride of `partial` per storage index (0: nt)
  // Dataflow schedule (k_chol_flow): one int per tile and storage index (row-major lower triangle, ntri per
  // particle), raised when the tile holds its final L(i,k); per-XCD ticket counters of the work queue.
  int* tflag;
  int ntri;
  int* qnext;
  long long* trace;     // optional (agp_debug_flow_trace): per item {start, end, wait} in 100 MHz ticks + {item info}
  int schur_diag_only;  // Schur mode: only the diagonal tiles of the prediction block (marginal variances + mean; no covariance)
  int lag;              // 1: sorted regular grid, the fused programs' stationary leaves are OP_LAG_* (GM = 2 instantiations)
  const double* lagtab; // ... and their tables (k_lag_tables)
  const int32_t* lagr;  // rank tables (sweeps in the caller's order; see cov_prologue): ranks of the resident points, null = sorted sweep
  int lag_stride;       // ... doubles per table
  CltArgs clt;          // compact tables (lagr then holds the points' keys; lag_stride = doubles per table in LDS)
  const double* noise_q; // fused evaluation: [P] noise on the prediction block's diagonal (see CovArgs), null = none
};
// LDS byte budget of the update kernel: GEMM double buffers and the potrf block store alias.
constexpr int U_SLAB = KB * LDS_STRIDE;                // doubles per slab buffer
constexpr int U_GEMM_DOUBLES = 4 * U_SLAB;             // As[2], Bs[2]      = 9216
constexpr int U_BLK_DOUBLES = (NSB * (NSB + 1) / 2) * 256;  // 36 blocks   = 9216
constexpr int U_MAIN_DOUBLES = (U_GEMM_DOUBLES > U_BLK_DOUBLES) ? U_GEMM_DOUBLES : U_BLK_DOUBLES;
// extras: rvec[128], avec[128] (alpha_k), xv[2][16] (alpha_j slab staging), Wl[256]
constexpr int U_EXTRA_DOUBLES = 128 + 128 + 64 + 256;
constexpr int U_LDS_BYTES = (U_MAIN_DOUBLES + U_EXTRA_DOUBLES) * 8;

// Largest number of ChangePoint nodes whose sigma tables fit the (aliased) LDS of the fused path.
// LDS map of the fused phase (aliases the slab buffers): tpt[256] | sig[n_cp][256] | prm[n_prm] | ops[n_ops] (int)
constexpr int U_MAX_CP = (U_MAIN_DOUBLES - 256 - 3 * AGP_MAX_OPS_DEV - AGP_MAX_OPS_DEV / 2 - 8) / 256;

constexpr int T_NBLK = NSB * (NSB - 1) / 2;              // 28 strictly-lower 16x16 blocks
constexpr int T_LDS_DOUBLES = (T_NBLK + NSB) * 256;      // + 8 inverse blocks = 72 KiB
static_assert(T_LDS_DOUBLES <= U_MAIN_DOUBLES, "solve staging must fit the aliased slab buffers");
struct GatherArgs {
  double* dstA; long long dst_strideA; const double* srcA; long long src_strideA; long long nA;      // doubles
  double* dstW; long long dst_strideW; const double* srcW; long long src_strideW; long long nW;
  double* dstV; long long dst_strideV; const double* srcV; long long src_strideV; long long nV;
  double* dstP; long long dst_strideP; const double* srcP; long long src_strideP; long long nP;      // log-det / quadratic-form partials (nP = 0: not wanted)
  const int* src_slot; int* ready; int nt1;
};
struct PredArgs {
  const double* A; long long strideA;
  const double* vec; int ldv;
  const double* mu2;        // [m] or null
  const double* noise_pred; // [P]
  const double* diag_add;   // [m] extra diagonal term per prediction point (infer_gp_sum) or null
  const uint8_t* np_code;   // [m] query codes (infer_gp_sum_batch) or null: noise_pred then goes on the code-0 rows only, after
                            // diag_add (A + 0 + (diag_add + noise_pred), the single entry's order); null: A + noise_pred + diag_add
  int nt1, n1_pad, m, P;
  double* out_mean;         // [P][m]
  double* out_var;          // [P][m]
  double* out_cov;          // [P][m*m] or null
};

// predict_sum's read-out (k_sum_readout, agp_sum_kernel.hpp)
struct SumReadArgs {
  double* mean;            // [P][m] in: predictive means (k_pred_extract), out: raw means
  const double* var;       // [P][m] predictive variances
  int m, p_rows;           // joint rows (M + 1) p; the F_1 rows are [0, p_rows)
  double slope, intercept, shift, ivar;      // y_transform; shift = intercept / slope; ivar = 1 / slope^2
  const double* z;         // [nq] ndtri(q)
  int nq;
  double* x;               // [P][m][nq]
  int32_t* bad;            // [P] smallest failing row + 1, or untouched
};

// posterior predictive samples (agp_sample_kernel.hpp).  Column j of Z / entry j of col is the j-th sample of the call in chunk order.
constexpr int SMP_G = 32;      // samples per workgroup of k_pred_sample
struct SampleNormArgs {
  double* Z;               // [m_pad][ldz] (row i, column j), 0 in padding rows and columns
  int m, m_pad, ldz, S;    // S live columns
  const int32_t* col;      // [S] sample index s of column j
  uint64_t seed;
  const double* zin;       // [S][m] the caller's normals z[s * m + i], or null: Philox4x64-10 + ndtri
};
struct SampleReadArgs {
  const double* A;         // the chunk's factors (packed lower tiles), particle q of the chunk at A + q strideA
  long long strideA;
  const double* vec;       // a = L11^-1 (x - mu1) in rows [0, n1_pad) of particle q's vector at vec + q ldv
  int ldv;
  const double* mu2;       // [m] or null
  const double* Z;         // SampleNormArgs::Z
  int ldz;
  const int32_t* col;      // [S] output column of column j
  const int32_t* grp;      // [groups][4]: {particle of the chunk, first column j0, columns (<= SMP_G), 0}
  int nt1, m;
  double zsign, slope, intercept;      // zsign = sign(slope)
  double* out;             // [S][m]
};

// mixture moments (agp_mixmom_kernel.hpp): one chunk of components in the pass's order, and the running sums about the pivot
struct MixMomArgs {
  const double* mean;      // [Pc][m] component means (the predictive's scaled space)
  const double* var;       // component p's variance at point i: var[p * v_pstride + i * v_istride] ([Pc][m], or the diagonals of cov)
  long long v_pstride, v_istride;
  const double* cov;       // [Pc][m*m] column-major symmetric, or null (marginal pass)
  const double* w;         // [Pc] weights
  int m, Pc, space;        // space 0: normal components, 1: MvLogNormal(N(mu_r, C_r))
  int pivot;               // >= 0: this chunk starts the sums, about the component mean of its particle `pivot`; < 0: it continues them
  double slope, intercept, ivar;      // mu_r = (mu - intercept) / slope, C_r = ivar * C (ivar = 1 / slope^2)
  double* e;               // [Pc][m] the components' means in the output space (k_mixmom_marginal writes, k_mixmom_cov reads)
  double* s;               // [m] pivot
  double* s1;              // [m] S1 = sum w (e - s)
  double* s2d;             // [m] diagonal of S2 (marginal pass)
  double* acc;             // [m*m] lower triangle of S2 = sum w (C + (e - s)(e - s)'), column-major
  double* out_mean;        // [m]
  double* out_var;         // [m]
  double* out_cov;         // [m*m] or null
};

struct GradArgs {
  const double* A;       // packed lower tiles of L
  double* Z;             // packed buffer holding Z(r,k), r <= k, in the slot of lower tile (k,r)
  long long strideA;
  const double* W;       // [P][nt][NSB][256] per-step 16x16 inverses
  const double* beta;    // [P][ldv]  L^-1 x
  double* alpha;         // [P][ldv]  K^-1 x
  int ldv;
  int P, nt, n;          // n = valid points (no prediction segment here)
  // gradient programs (device order; see GProgHdr)
  const struct GProgHdr* ghdr;
  const uint8_t* gops;   // opcode per node
  const uint8_t* glc;    // left / right child node index per node (binary nodes)
  const uint8_t* grc;
  const int32_t* gpoff;  // per node: offset of its parameters inside the particle's parameter block
  const double* gprm;    // ORIGINAL (untransformed-by-us) parameter values, device node order
  const double* tt;      // time points (padded)
  const double* logdt;   // log|dt| table of the resident data (null: GammaExp leaves compute the power); see CovArgs
  double* gpart;         // [P][ntiles][csplit][gstride] per-tile partial sums (slot 0..n_prm-1 params, n_prm = noise)
  int gstride;
  int csplit;            // k_grad_contract: workgroups per tile (grid.z; 1, or 4 in sweeps with fewer tiles than workgroup slots)
  const int32_t* gmap;   // per particle parameter slot -> index in the caller's parameter array
  const int32_t* out_off;   // [P] offset of the particle's gradient block in out_grad (caller order, via map)
  const int32_t* pmap;   // sorted particle -> caller particle
  const int32_t* plist;  // k_grad_contract / k_lag_grad: particles of this launch (indices into the sorted group)
  int tape_off;          // k_grad_contract<0>: offset (doubles) of the LDS tape inside the dynamic shared memory
  // resident factors (nullable): particle p with lslot[p] >= 0 reads L and the inverse blocks from the factor store
  // (slot lslot[p]; Lstride doubles per slot, Wnt block columns per slot) instead of A / W — nothing is copied
  const int32_t* lslot; const double* Lsrc; long long Lstride; const double* Wsrc; int Wnt;
  double* out_grad;
  double* out_gnoise;
  // lag-domain contraction (regular time grids; see k_lag_grad): rank of every resident point in the sorted series, the sorted
  // series itself, number of lag bins (= resident points), reference time of the Linear moments
  const int32_t* rank; const double* tts; int nbins; double tref;
  const double* tw;      // exp(-2 pi i k / 4096), k = 0 .. 4095, (re, im) pairs (k_zspec / k_lag_grad)
  const int32_t* klist; int kn;      // k_kinv_tiles: the particles whose K^-1 tiles are wanted (null: all P)
  double grid_h, grid_mid;           // regular grid: spacing, and the (fractional) rank of t_ref: t_sorted[r] - t_ref = (r - grid_mid) h
  long long strideZ;                 // doubles per particle in Z (0: strideA)
  double* dinv;                      // [P][ldv] diag(K^-1) = row sums of squares of Z (k_trtri_chain; null: not wanted)
  // resident L^-T (predictive passes that start from the factor store): particle p with lslot[p] >= 0 keeps its Z in the store's
  // slot (Zstride doubles per slot) together with the running alpha and diag(K^-1) of its rows ([slot][zld]); the first zi0[p] tile
  // columns are there already — Z(j, i) for i < zi0 — and only the new columns are formed (null Zsrc: none of this; zi0[p] < 0: a copy of
  // another particle of the sweep with the same slot — it forms its Z in the sweep's scratch and leaves the slot alone)
  // zfull = floor(n / 128): the complete tile columns, the only ones a slot's running sums and its resident-column count cover
  double* Zsrc; long long Zstride; const int32_t* zi0; double* zalpha; double* zdinv; long long zld; int zfull;
  // Toeplitz variant of the lag-domain particles (k_toep_solve / k_lag_grad): K^-1 [e_first, 1, t - t_ref] per particle
  // ([P][3][ldv]), and the rank of the sweep's first point in time (its points occupy ranks rank0 .. rank0 + n - 1)
  double* tsol; int rank0;
  const double* noise;               // [P] observation noise of the group's particles
  double poly_mmax;                  // bound of |midpoint| over the resident series (fixed-point scale of the moment histograms)
  double toep_max_amp;               // largest accepted entry of U' T^-1 U C (k_lag_grad)
  int32_t* retry;                    // [caller's P] set when the Linear leaves' downdate is too ill-conditioned: the host repeats that particle with L^-T
};

struct GProgHdr {
  int32_t node_off;   // offset into gops / glc / grc / gpoff
  int32_t prm_off;    // offset into gprm / gmap
  int32_t n_ops;
  int32_t n_prm;
  int32_t n_cp;
  int32_t flags;      // bit 0: the tree has GammaExp leaves (reads the log|dt| table when there is one)
                      // bit 1: lag-domain contraction (k_kinv_tiles bins G by lag, k_lag_grad differentiates n lags instead of n^2 elements)
};
                      // bit 2 (with bit 1): the lag sums of K^-1 come from the power spectrum of Z's columns (k_zspec), no K^-1 tiles at all
constexpr int GFLAG_LAGDOM = 2;
constexpr int GFLAG_LAGFFT = 4;
                      // bit 3 (with bit 1): the sweep's points are n consecutive grid points, so K = Toeplitz + the Linear leaves' rank-2
                      // term: the lag sums of K^-1 follow from four solves with L (Gohberg-Semencul) — no L^-T, no K^-1 tiles
constexpr int GFLAG_LAGTOEP = 8;
                      // bit 4: Linear leaves inside products (at most d = bits 8-9 of them along any product path, no ChangePoint): at a
                      // fixed lag the kernel is a polynomial of degree 2d in the pair's midpoint m = (t_a + t_b)/2 - t_ref, so
                      // sum_ab G_ab dK_ab = sum over lags and 2d+1 probe midpoints of [moment-matched weights] x dK(probe):
                      // k_kinv_tiles bins G m^k (k = 0..2d) by lag, k_lag_grad differentiates (2d+1) n virtual elements
constexpr int GFLAG_LAGPOLY = 16;
                      // bit 5 (with bits 1, 3): tsol holds T^-1 [x, e_first, 1, t - t_ref] in SORTED coordinates (structured gradient sweep:
                      // Schur recursion + backward substitution, no dense factor): no downdate, alpha is formed in k_lag_grad
constexpr int GFLAG_LAGTSOL = 32;
constexpr int GFLAG_POLY_DEG_SHIFT = 8;
constexpr int LAGDOM_MAX_BINS = 4096;      // LDS histogram of k_kinv_tiles (32 KiB)
constexpr int FFT_N = 4096;                // transform length of the spectral variant: series of up to FFT_N / 2 points

constexpr int LDS_TAPE_NODES = 8;
constexpr int FFT_BUF = FFT_N + FFT_N / 16;

// Small-matrix value kernel (k_series_logpdf, agp_series_kernel.hpp): one workgroup per particle, the particle's whole series in LDS.
constexpr int SERIES_MAX_N = 176;                 // == AGP_SERIES_MAX_N of the C ABI (agp_series.hip checks)
constexpr int SERIES_LDS_BYTES = 160 * 1024;      // what one workgroup may declare on gfx950
struct SeriesArgs {
  const double* ts;          // S series, concatenated: series s is [pt_off[s], pt_off[s + 1])
  const double* xs;
  const long long* pt_off;   // [S + 1]
  const int32_t* series;     // [P] series of particle p
  const int32_t* wg;         // [grid] particle of workgroup b of this launch (longest series first)
  const ProgHdr* hdr;        // [P] programs compiled without tables of the resident series (no OP_GE_TAB, no OP_LAG)
  const uint8_t* ops;
  const double* prm;
  const double* noise;       // [P]
  double* out_lp;            // [P]
  int32_t* out_info;         // [P]
};
// LDS map of one workgroup, in doubles, from the particle's own sizes alone (the launch declares the largest total of its particles;
// where a workgroup's arrays sit never depends on what else is in the launch):
//   Wl[256] | tpt[np] | rvec[np] | avec[np] | etab[128] | prm[n_prm + 2, even] | ops[n_ops ints, even] | sig[n_cp][256] | blocks
// np = 16 nb points, nb = ceil(n / 16) block rows, nb (nb + 1) / 2 lower 16 x 16 blocks of 256 doubles.
struct SeriesLds {
  int nb, np, o_tpt, o_rvec, o_avec, o_etab, o_prm, o_ops, o_sig, o_blk, total;      // offsets and total in doubles
};
__host__ __device__ inline SeriesLds series_lds(int n, int n_ops, int n_prm, int n_cp) {
  SeriesLds m;
  m.nb = (n + BS - 1) / BS; m.np = m.nb * BS;
  m.o_tpt = 256; m.o_rvec = m.o_tpt + m.np; m.o_avec = m.o_rvec + m.np; m.o_etab = m.o_avec + m.np;
  m.o_prm = m.o_etab + 128;
  m.o_ops = m.o_prm + ((n_prm + 3) & ~1);
  m.o_sig = m.o_ops + (((n_ops + 1) / 2 + 1) & ~1);
  m.o_blk = m.o_sig + n_cp * 256;
  m.total = m.o_blk + (m.nb * (m.nb + 1) / 2) * 256;
  return m;
}

// Value-and-gradient twin (k_series_logpdf_grad, agp_logpdf_grad_series_batch): the value kernel's arguments, the particles' gradient
// programs (compile_batch's tables, caller's order) and the gradient outputs.
struct SeriesGradArgs : SeriesArgs {
  const GProgHdr* ghdr;      // [P]
  const uint8_t* gops;       // opcode / left child / right child per node
  const uint8_t* glc;
  const uint8_t* grc;
  const int32_t* gpoff;      // per node: offset of its parameters inside the particle's parameter block
  const double* gprm;        // original parameter values, node order (three doubles of tail padding)
  const int32_t* gmap;       // per parameter slot -> index in the caller's parameter block of the particle
  const int32_t* out_off;    // [P] offset of the particle's block in out_grad (the caller's prm_off)
  double* out_grad;          // [prm_off[P]]
  double* out_gnoise;        // [P]
};
// LDS map of the gradient kernel: the value kernel's arrays at the value map's offsets up to the per-point tables, then — in front
// of the blocks —
//   csig[n_cp][256] (1 - sigma of every ChangePoint node, directly behind sig) | alpha[np] | gprm[g_n_prm + 3, even] | gpoff[g_n_ops ints] ops, lc, rc, mv[g_n_ops bytes each] (g_n_ops doubles, even) |
//   red[4][g_n_prm + 1] (even) | blocks
// i.e. 256 n_cp + np + 5 g_n_prm + g_n_ops + ~8 doubles more than series_lds: 2.1 KiB at 176 points beside a tree of 5 nodes and 9
// parameters, and 2 KiB more per ChangePoint node.
struct SeriesGradLds : SeriesLds {
  int o_alpha, o_gprm, o_gtab, o_red;
};
__host__ __device__ inline SeriesGradLds series_grad_lds(int n, int n_ops, int n_prm, int n_cp, int g_n_ops, int g_n_prm) {
  SeriesGradLds m;
  static_cast<SeriesLds&>(m) = series_lds(n, n_ops, n_prm, n_cp);
  m.o_alpha = m.o_blk + n_cp * 256;      // (csig sits at the value map's o_blk = o_sig + n_cp * 256)
  m.o_gprm = m.o_alpha + m.np;
  m.o_gtab = m.o_gprm + ((g_n_prm + 4) & ~1);
  m.o_red = m.o_gtab + ((g_n_ops + 1) & ~1);
  m.o_blk = m.o_red + ((4 * (g_n_prm + 1) + 1) & ~1);
  m.total = m.o_blk + (m.nb * (m.nb + 1) / 2) * 256;
  return m;
}

// HMC twin (k_series_hmc, agp_hmc_series_batch): the gradient kernel's arguments — its programs are compiled from the INITIAL state
// and give the structure only; the device derives every parameter value from the latent state before each evaluation — the latent
// state, the transform classes, the move schedule and the chain outputs.  Per-parameter arrays have the caller's layout (out_off).
struct SeriesHmcParams {
  const double* z;           // [prm_off[P]] latent coordinates (a FIXED slot: the parameter value itself)
  const double* z_noise;     // [P]
  const int32_t* cls;        // [prm_off[P]] transform class of every caller parameter, < 0: FIXED
  const uint8_t* rule;       // per gradient-program parameter slot (gprm's layout): how the VALUE program's slot follows from the
                             // caller parameter gmap names — HMC_RULE_* (the value and the gradient program number their slots alike)
  const double* tf;          // [C][3] (mu, sigma, scale); scale == 0: log-normal, > 0: logit-normal
  int C, noise_class;
  double noise_jitter;
  int n_hmc, L_prm, L_noise, n_exit, flags;      // flags: HMC_FLAG_*
  double eps_prm, eps_noise;
  const unsigned long long* seeds;               // [P] Philox key (seeds[p], 0)
  double* out_z;             // [prm_off[P]]
  double* out_z_noise;       // [P]
  double* out_prm;           // [prm_off[P]] transformed parameters of the final state
  double* out_noise;         // [P]
  int32_t* out_counts;       // [P][4] parameter moves accepted, tried, noise moves accepted, trajectories rejected as not positive definite
  double* out_trace;         // [P][n_hmc][2][2] (alpha, log u) of every move, NaN where none was made; or null
};
// (the chain's own arguments sit in device memory behind one pointer: the evaluation's statements keep the gradient kernel's
// argument block and its scalar registers; the chain reads a field where it needs it)
struct SeriesHmcArgs : SeriesGradArgs {
  const SeriesHmcParams* hm;
  int C;                     // == hm->C (the LDS map needs it)
};
constexpr int HMC_RULE_COPY = 0, HMC_RULE_INV_SQ = 1, HMC_RULE_INV = 2, HMC_RULE_M2_INV_SQ = 3, HMC_RULE_PI_OVER = 4;
constexpr int HMC_FLAG_FULL_NOISE_GRAD = 1;      // measurement: noise moves run the whole gradient pass (no tr K^-1 = |Z|_F^2 shortcut)
constexpr unsigned long long HMC_PHILOX_TAG = 0x484D43ull;      // counter word c3 of every draw ("HMC")
// compiled value of a value-program slot from the caller parameter v — the operations of emit (agp_engine.hip), IEEE division
__host__ __device__ inline double hmc_rule_apply(int rule, double v) {
  switch (rule) {
    case HMC_RULE_INV_SQ: return 1.0 / (v * v);
    case HMC_RULE_INV: return 1.0 / v;
    case HMC_RULE_M2_INV_SQ: return -2.0 / (v * v);
    case HMC_RULE_PI_OVER: return 3.14159265358979323846 / v;
    default: return v;
  }
}
// LDS map of the HMC kernel: the gradient kernel's, and in front of the blocks six doubles per caller parameter (npc of them, =
// g_n_prm: gmap is a permutation) and the chain's scalars —
//   theta[npc] (the caller-order vector) | z[npc] | zs[npc] (saved) | mom[npc] | grd[npc] (gradient in caller order) |
//   cls[npc ints] smap[npc ints] (gmap | rule << 16) | tf[3 C] (even) | st[HMC_ST_N] | blocks
// At 176 points a chain of 4 ChangePoint nodes (9 nodes, 13 parameters, 8 tables) still fits, as in the gradient kernel; 5 do not.
constexpr int HMC_ST_N = 32;
struct SeriesHmcLds : SeriesGradLds {
  int o_th, o_z, o_zs, o_mom, o_grd, o_cls, o_tf, o_st;
};
__host__ __device__ inline SeriesHmcLds series_hmc_lds(int n, int n_ops, int n_prm, int n_cp, int g_n_ops, int g_n_prm, int C) {
  SeriesHmcLds m;
  static_cast<SeriesGradLds&>(m) = series_grad_lds(n, n_ops, n_prm, n_cp, g_n_ops, g_n_prm);
  const int npc = (g_n_prm + 1) & ~1;
  m.o_th = m.o_blk; m.o_z = m.o_th + npc; m.o_zs = m.o_z + npc; m.o_mom = m.o_zs + npc; m.o_grd = m.o_mom + npc;
  m.o_cls = m.o_grd + npc;
  m.o_tf = m.o_cls + npc;
  m.o_st = m.o_tf + ((3 * C + 1) & ~1);
  m.o_blk = m.o_st + HMC_ST_N;
  m.total = m.o_blk + (m.nb * (m.nb + 1) / 2) * 256;
  return m;
}

// Predictive twin (k_series_predict, agp_predict_series_batch): the value kernel's arguments, every series' own query times and
// the particle-major outputs.
struct SeriesPredArgs : SeriesArgs {
  const long long* q_off;    // [S + 1] series s predicts at ts_pred[q_off[s] .. q_off[s + 1])
  const double* ts_pred;
  const double* noise_pred;  // [P]
  const long long* out_off;  // [P + 1] particle p's block in out_mean / out_var
  double* out_mean;          // [out_off[P]]
  double* out_var;
};
// LDS map of the predictive kernel: the value kernel's, array for array — the finished query blocks live in registers, the query
// times come straight from memory, and sigma_cp of a wave's current 16 query times sits in entries SERIES_QSLOT + 16 w .. + 15 of
// every per-point table, past the at most SERIES_MAX_N entries a series uses.  So the need, and with it the number of ChangePoint
// tables that fit, is the value entry's.  n = 0 (the prior predictive) is a map without points or blocks.
constexpr int SERIES_QSLOT = 192;
static_assert(SERIES_QSLOT >= SERIES_MAX_N && SERIES_QSLOT + 4 * 16 <= 256, "four waves' query entries behind the series' own");
__host__ __device__ inline SeriesLds series_pred_lds(int n, int n_ops, int n_prm, int n_cp) { return series_lds(n, n_ops, n_prm, n_cp); }

// Decomposition twin (k_series_predict_sum, agp_predict_sum_series_batch): the predictive twin's arguments on COMPOSITE programs
// (K_1 SEL_1 * K_2 SEL_2 * + ..: append_composite) and coded joint rows.  Series s with m query times has (M + 1) m rows g in the
// order F_1(T*) .. F_M(T*), X(T*): row g is component i = g / m at time ts_pred[q_off[s] + g % m], code i < M ? i + 1 : 0, diagonal
// addend 1e-8 + (i == M ? noise_pred[p] : 0).  out_off counts ROWS ((M + 1) times the predictive twin's); out_mean / out_var take the
// raw-space marginals of predict_sum (k_sum_readout's statements) and out_x their nq Normal quantiles per row.  The LDS map is
// series_pred_lds with the M selector tables counted in n_cp (ProgHdr::n_cp does): a query row's selector entries sit in the
// tables' entries SERIES_QSLOT .. like sigma_cp's.
struct SeriesSumArgs : SeriesPredArgs {
  int M, nq;
  const double* y_slope;     // [S]
  const double* y_intercept; // [S]
  const double* z;           // [nq] ndtri(q[k]), from the host
  double* out_x;             // [nq out_off[P]] row-major (row, k); unused when nq == 0
};

// Held-out twin (k_series_predict_logpdf, agp_predict_logpdf_series_batch): the value kernel's arguments, every series' own query
// times and held-out values, and the outputs.  The workgroup factors the JOINT matrix of the series' n training points followed —
// without padding — by its m query points, N = n + m <= SERIES_MAX_N, in the value kernel's LDS map at N points (series_lds(N, ..)),
// and reads the query rows' partials: the need, the LDS classes and the host's refusal rule are the value entry's at N.
struct SeriesProbaArgs : SeriesArgs {
  const long long* q_off;    // [S + 1] series s is scored at ts_pred[q_off[s] .. q_off[s + 1])
  const double* ts_pred;
  const double* y_pred;      // [q_off[S]] held-out values, in the space of xs
  const double* noise_pred;  // [P] the diagonal addend of the query rows
  const double* y_slope;     // [S] the Jacobian term: + m log|y_slope[s]| (1: none)
  const long long* out_off;  // [P + 1] particle p's block in out_terms
  double* out_terms;         // [out_off[P]] or null: the per-point (prequential) terms
};

// Sampling twin (k_series_predict_sample, agp_predict_sample_series_batch): the held-out twin's arguments (y_pred and out_terms
// unused: the query rows' right-hand side is 0) and the read-out of the query rows of the joint factor — samples, component means
// and covariances in the raw space of every series' own transform.
struct SeriesSampleArgs : SeriesProbaArgs {
  const double* y_intercept;         // [S]
  long long R;                       // samples per series
  const unsigned long long* seeds;   // [S] Philox key (seeds[s], 0) of series s
  const double* zin;                 // [R q_off[S]] the caller's normals in out_x's layout, or null: Philox4x64-10 + ndtri
  const long long* smp_off;          // [P + 1] particle p's samples: smp[smp_off[p] .. smp_off[p + 1]), ascending
  const int32_t* smp;                // [samples of all series] index j in [0, R) inside the particle's series
  double* out_x;                     // [R q_off[S]] series s at R q_off[s], sample j at + j m_s
  double* out_mean;                  // [out_off[P]] or null
  const long long* cov_off;          // [P + 1] particle p's m_s x m_s block in out_cov
  double* out_cov;                   // [cov_off[P]] or null
};
// The read-out behind it (k_series_sample_fill): series s's whole block of out_x becomes NaN when one of its particles
// plist[pl_off[s] ..] has a non-zero info word.
struct SeriesSampleFillArgs {
  int S;
  long long R;
  const long long* q_off;    // [S + 1]
  const long long* pl_off;   // [S + 1]
  const int32_t* plist;      // [P]
  const int32_t* info;       // [P] the kernel's out_info (written for every particle of a series with query points)
  double* out_x;
};

// The mixture read-out of agp_predict_logpdf_series_batch (k_series_mix_logp, agp_series_quantile_kernel.hpp): series s's particles
// plist[pl_off[s] ..] (ascending caller index) with the weights w[w_off[s] + j] — quant_plan's lists, as SeriesQuantArgs reads them.
struct SeriesMixLogpArgs {
  int S;
  const long long* q_off;    // [S + 1]
  const long long* pl_off;   // [S + 1]
  const long long* w_off;    // [S + 1]
  const int32_t* plist;      // [P]
  const double* w;           // [w_off[S]]
  const double* lp;          // [P] the kernel's out_lp (written for every particle of a series with held-out points)
  const int32_t* info;       // [P]
  double* out;               // [S]
};

// The read-out of agp_predict_quantile_series_batch (agp_series_quantile_kernel.hpp) on the predictive launches' device outputs.
// Series s's mixture: its P_s = pl_off[s + 1] - pl_off[s] particles plist[pl_off[s] ..] (ascending caller index), their weights
// w[w_off[s] + j] padded with 0 to Pp_s = w_off[s + 1] - w_off[s] = ceil(P_s / 64) 64, and the packed rows of its m_s query points,
// row i at row_off[s] + i Pp_s of cm / cs: entry j = particle j's raw mean / standard deviation, (0, 1) in the padding.
struct SeriesQuantArgs {
  int S, nq;
  const long long* pt_off;   // [S + 1]
  const long long* q_off;    // [S + 1]
  const long long* out_off;  // [P + 1] particle p's block in mean / var (SeriesPredArgs::out_off)
  const double* mean;        // the predictive's outputs (scaled space)
  const double* var;
  const int32_t* pred_info;  // [P] the predictive's info words (written for every launched particle: n_s > 0 or m_s > 0)
  const long long* pl_off;   // [S + 1]
  const long long* w_off;    // [S + 1]
  const long long* row_off;  // [S + 1]
  const int32_t* plist;      // [P]
  const double* w;           // [w_off[S]]
  const double* slope;       // [S] y_transform of series s: raw mean = (mu - intercept) / slope, raw variance = ivar * var
  const double* intercept;   // [S]
  const double* ivar;        // [S] 1 / slope^2
  const double* q;           // [nq]
  double tol;
  long long max_iter;
  double* cm;                // [row_off[S]]
  double* cs;
  int32_t* first_bad;        // [P] 0, or n_s + i + 1 for the first query i whose raw mean is not finite or raw variance negative / NaN
  int32_t* bad;              // [S] some particle of the series has no predictive or a first_bad word (series with particles only)
  double* out_x;             // [nq q_off[S]] series s's (nq, m_s) row-major block at nq q_off[s]
  int32_t* out_conv;
  int32_t* out_iters;
  double* out_mean;          // [q_off[S]] or null: the mixture's marginal moments
  double* out_var;
};

// Long-series value kernel (k_long_series_logpdf, agp_long_series_kernel.hpp, agp_logpdf_long_series_batch): one workgroup per
// particle of a series of up to LONG_SERIES_MAX_N points; the factor lives in an HBM workspace, LDS holds vectors, tables and ONE
// diagonal block.  The value kernel's arguments and the workspace: workgroup b of a launch owns ws[b * ws_stride ..), ws_stride >=
// 256 nb (nb + 1) / 2 doubles for every particle of the launch.
constexpr int LONG_SERIES_MAX_N = 512;            // == AGP_LONG_SERIES_MAX_N of the C ABI (agp_series.hip checks)
constexpr int LONG_SIG_STRIDE = 512;              // entries of one per-point table: the whole series, indexed by the point's position
struct LongSeriesArgs : SeriesArgs {
  double* ws;
  long long ws_stride;       // doubles per workgroup
};
// LDS map of one workgroup, in doubles, from the particle's own sizes alone:
//   Wl[256] | dblk[256] | tpt[np] | rvec[np] | avec[np] | ldg[np] | etab[128] | prm[n_prm + 2, even] | ops[n_ops ints, even] | sig[n_cp][512]
// Wl = inverse of the current diagonal block, dblk = that block, ldg = 2 log L_ii per row.  At 512 points: 4 KiB + 16 KiB + 1 KiB
// + the program + 4 KiB per ChangePoint node — 61 KiB beside 10 nodes (two workgroups share a CU); the 160 KiB one workgroup may
// declare hold 34 nodes beside a small program.
struct LongSeriesLds {
  int nb, np, o_dblk, o_tpt, o_rvec, o_avec, o_ldg, o_etab, o_prm, o_ops, o_sig, total;      // offsets and total in doubles
};
__host__ __device__ inline LongSeriesLds long_series_lds(int n, int n_ops, int n_prm, int n_cp) {
  LongSeriesLds m;
  m.nb = (n + BS - 1) / BS; m.np = m.nb * BS;
  m.o_dblk = 256; m.o_tpt = 512; m.o_rvec = m.o_tpt + m.np; m.o_avec = m.o_rvec + m.np; m.o_ldg = m.o_avec + m.np;
  m.o_etab = m.o_ldg + m.np;
  m.o_prm = m.o_etab + 128;
  m.o_ops = m.o_prm + ((n_prm + 3) & ~1);
  m.o_sig = m.o_ops + (((n_ops + 1) / 2 + 1) & ~1);
  m.total = m.o_sig + n_cp * LONG_SIG_STRIDE;
  return m;
}

// Long-series predictive twin (k_long_series_predict, agp_predict_long_series_batch): the short predictive twin's arguments and the
// workspace.  Stage P's query blocks (16 times each) run in rounds of LONG_PRED_C blocks per wave.  Workspace of a particle with
// nb block rows, in blocks of 256 doubles:
//   rows 0 .. nb - 1 of the packed triangle | rows nb .. nb + 4 LONG_PRED_C - 1 of the same packing: the round's scratch rows, row
//   nb + w + 4 u is chain u of wave w (blocks 0 .. nb - 1: VT(q, k); block nb: k(t*, t*)) | nb blocks W(j) = L(j, j)^-1
// — long_series_pred_ws_blocks(nb); it does not grow with the number of query times.  ws_stride >= 256 times that for every
// particle of the launch.
constexpr int LONG_PRED_C = 2;
constexpr int LONG_PRED_QSLOT = LONG_SERIES_MAX_N;      // per-point tables: the round's query entries behind the series' own
constexpr int LONG_PRED_SIG_STRIDE = LONG_PRED_QSLOT + 4 * LONG_PRED_C * 16;
struct LongSeriesPredArgs : SeriesPredArgs {
  double* ws;
  long long ws_stride;       // doubles per workgroup
};
__host__ __device__ inline long long long_series_ws_blocks(int nb) { return (long long)nb * (nb + 1) / 2; }
__host__ __device__ inline long long long_series_pred_ws_blocks(int nb) { return long_series_ws_blocks(nb + 4 * LONG_PRED_C) + nb; }
// LDS map: the value kernel's, array for array, with per-point tables of LONG_PRED_SIG_STRIDE entries — sigma_cp of chain u of wave
// w at its 16 query times sits in entries LONG_PRED_QSLOT + 16 (LONG_PRED_C w + u) .. + 15.  At 512 points: 21 KiB + the program + 5
// KiB per ChangePoint node — 71 KiB beside 10 nodes (two workgroups still share a CU); 160 KiB hold 27 nodes beside a small program.
__host__ __device__ inline LongSeriesLds long_series_pred_lds(int n, int n_ops, int n_prm, int n_cp) {
  LongSeriesLds m = long_series_lds(n, n_ops, n_prm, 0);
  m.total = m.o_sig + n_cp * LONG_PRED_SIG_STRIDE;
  return m;
}

// Long-series held-out twin (k_long_series_predict_logpdf, agp_predict_logpdf_long_series_batch): the short held-out twin's arguments
// and the workspace.  The workgroup factors the JOINT matrix of the series' n training points followed — without padding — by its m
// query points, N = n + m <= LONG_SERIES_MAX_N, in the long value kernel's LDS map and workspace at N points (long_series_lds(N, ..),
// long_series_ws_blocks(ceil(N / 16))), and reads the query rows' partials: need, classes, chunks and the host's refusal rule are
// the long value entry's at N.
struct LongSeriesProbaArgs : SeriesProbaArgs {
  double* ws;
  long long ws_stride;       // doubles per workgroup
};

// Arguments of the probe instantiation k_series_logpdf<D, true> (agp_debug_series_factor): caller matrices of ONE size take the place
// of series, programs and noise; the LDS map is series_lds(n, 0, 0, 0); workgroup b factors matrix b.
struct SeriesProbeArgs {
  const double* K;           // [P][n][n] row-major; only the lower triangle is read
  const double* y;           // [P][n] right-hand sides, or null (zeros)
  int n;
  double* out_blk;           // [P][nb (nb + 1) / 2][256] the packed blocks as the factorisation leaves them
  double* out_alpha;         // [P][np] avec
  double* out_part;          // [P][2] 2 sum log L_ii, alpha'alpha
  double* out_lp;            // [P]
  int32_t* out_info;         // [P]
};

// Arguments of the probe instantiation k_long_series_logpdf<D, true> (agp_debug_long_series_factor): caller matrices of ONE size
// take the place of series, programs and noise; the LDS map is long_series_lds(n, 0, 0, 0); workgroup b factors matrix b in
// ws[b * ws_stride ..), which is the packed-block output as well.
struct LongSeriesProbeArgs {
  const double* K;           // [P][n][n] row-major; only the lower triangle is read
  const double* y;           // [P][n] right-hand sides, or null (zeros)
  int n;
  double* ws;                // [P][ws_stride] the packed blocks as the factorisation leaves them
  long long ws_stride;       // doubles per workgroup, >= 256 nb (nb + 1) / 2
  double* out_alpha;         // [P][np] avec
  double* out_part;          // [P][2] 2 sum log L_ii, alpha'alpha
  double* out_lp;            // [P]
  int32_t* out_info;         // [P]
};

// k_poison_rows (NaN-poison mode of the store's sweeps): per buffer b, slot u's doubles [row start(i0[u]), pitch) in slot[u]
struct PoisonRowsArgs {
  double* base[4];
  long long pitch[4];        // doubles per slot
  long long unit[4];         // doubles per tile row (A: per tile)
  int tri[4];                // 1: packed lower triangle (row i starts at tile i(i+1)/2)
  int nt_cap;
  const int* slot;
  const int* i0;
};
}  // namespace agp
