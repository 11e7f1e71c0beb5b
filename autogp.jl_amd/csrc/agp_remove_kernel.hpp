// Removal of observations from a resident factor (agp_remove_data; remove_data!, src/api.jl:449-468 of the reference).
//
// Deleting the contiguous run [a, b) of r = b - a positions from a factored series leaves the rows of L before a as they are;
// of the rows from b on, the columns < a only move up; the trailing triangle S = L[b:, b:] is replaced by S' with
//     S' S'^T = S S^T + W W^T,   W = L[b:, a:b],
// a rank-r UPDATE: [S | W] Q = [S' | 0] with Q orthogonal (an LQ factorisation of the triangular-pentagonal matrix [S | W]).
// Row j's Householder reflector H_j = I - tau_j u_j u_j^T, u_j = [e_j; v_j], folds W[j, :] into the diagonal entry S[j][j]; it
// touches column j of S and all of W, and of those only the rows below j.  The new diagonal is taken POSITIVE directly
// (beta = +sqrt(S_jj^2 + |W_j|^2), tau = |W_j|^2 / ((S_jj + beta) beta), v = -W_j (S_jj + beta) / |W_j|^2: no cancellation since
// S_jj > 0), because everything downstream takes log L_ii and inverts the pivot blocks.  A row of W that is zero gives the
// identity (tau = 0), so the columns of the first touched tile that lie before a, and the identity padding of the last tile row,
// pass through unchanged; so does a row of W that is negligible against S_jj (RM_NEGLIGIBLE).
//
// The forward-solve vector rides along as one more row: with alpha = L^-1 x, the new trailing part solves
// S' alpha' = [S | W] [alpha_trail; alpha_run], i.e. [alpha'^T | *] = [alpha_trail^T | alpha_run^T] Q.
//
// Everything is written on the NEW tile grid: element (i, j) of the updated factor reads the old factor at (o(i), o(j)),
// o(k) = k < a ? k : k + r, and goes into a workspace in the store's packed layout (tile rows >= J0 = a / 128 only); k_rm_commit
// moves the workspace into the slot when all columns are done.  Per tile column J of the new trailing triangle:
//   k_rm_panel   one workgroup per particle: the reflectors of the diagonal tile (128 sequential steps, one barrier each; a row is
//                owned by two adjacent lanes that hold its W entries in registers), v_j / tau_j to global memory for the tiles
//                below, the new alpha_J, the log-det / quadratic-form partials, the inverses of the 16 x 16 pivot blocks, info;
//   k_rm_apply   one workgroup per (tile I > J, particle): the 128 reflectors applied to the rows of [S_IJ | W_I] — rows are
//                independent, so there is no barrier inside a 32-column chunk.
// A pass handles at most RM_RMAX columns of W (registers: RM_RMAX / 2 doubles per lane); a wider run takes several passes, the
// later ones in place on the workspace (shift 0).  The flops of a reflector applied row by row are 4 r per element of S against
// 2 (128 + 2 r) for the compact-WY products, and fp64 MFMA has the VALU's rate on gfx950: for the run widths a pass handles the
// element-wise form is the cheaper one and is bound by the tile traffic.
#pragma once
#include "agp_common.hpp"

namespace agp {

constexpr int RM_CW = 32;              // columns of a tile staged in LDS at a time
constexpr int RM_LDS = RM_CW + 1;      // row stride of the staged chunk (doubles): rows 2 banks apart, conflict-free 8-byte reads
constexpr int RM_RMAX = 32;            // columns of W one pass handles
constexpr double RM_NEGLIGIBLE = 1e-40;  // a row of W below 1e-20 |S_jj| is left alone: folding it would change nothing at 1e-20 relative, and the
                                         // reflector's scale 1 / |W_j|^2 overflows for the underflowed entries of a fast-decaying kernel's factor
constexpr int RM_VSTRIDE = NB * RM_RMAX + NB;      // doubles of reflector storage per particle: v_j (width of the pass) x 128, tau x 128

struct RemoveArgs {
  // the store (slot-indexed)
  double* A; long long strideA;
  double* Winv; int wsteps;
  double* vec; int ldv;
  double* partial; int ntp;
  int* info;
  const int* slot;                     // slot of particle p of this chunk
  // workspace (chunk-indexed)
  double* ws; long long ws_stride;     // tile rows [J0, nt_new) of the updated factor, packed; off0 = tile_off(J0, 0)
  long long off0;
  double* Wk; int ldw;                 // [RM_RMAX][ldw = nt_new * 128]: the pass's columns of W on the new row grid
  double* G; int ldg;                  // [r]: the run's entries of alpha, carried through the passes
  double* V;                           // [RM_VSTRIDE]: reflectors of the current tile column
  int a, r, n_new, nt_new, J0;
  int c0, rc;                          // the pass's columns [c0, c0 + rc) of the run
  int first, last;                     // first pass: reads the slot at shift r; later passes: the workspace in place
  int J;
};

__device__ __forceinline__ double rm_src(const RemoveArgs& g, const double* __restrict__ As, const double* __restrict__ wsp, int i, int j) {
  if (g.first) {
    const int oi = i < g.a ? i : i + g.r, oj = j < g.a ? j : j + g.r;
    return As[tile_off(oi >> 7, oj >> 7) + (long long)(oj & 127) * NB + (oi & 127)];
  }
  return wsp[tile_off(i >> 7, j >> 7) - g.off0 + (long long)(j & 127) * NB + (i & 127)];
}

// W of the pass on the new row grid (zero before a and in the padding), and on the first pass the run's alpha entries
__global__ __launch_bounds__(256) void k_rm_init(RemoveArgs g) {
  const int tid = threadIdx.x, p = blockIdx.y, ps = g.slot[p], I = g.J0 + blockIdx.x;
  const double* __restrict__ As = g.A + (long long)ps * g.strideA;
  double* __restrict__ Wkp = g.Wk + (long long)p * RM_RMAX * g.ldw;
  for (int idx = tid; idx < NB * RM_RMAX; idx += 256) {
    const int c = idx >> 7, i = I * NB + (idx & 127);
    double v = 0.0;
    if (c < g.rc && i >= g.a && i < g.n_new) {
      const int oi = i + g.r, oj = g.a + g.c0 + c;
      v = As[tile_off(oi >> 7, oj >> 7) + (long long)(oj & 127) * NB + (oi & 127)];
    }
    Wkp[(long long)c * g.ldw + i] = v;
  }
  if (g.first && blockIdx.x == 0) {
    const double* __restrict__ vecp = g.vec + (long long)ps * g.ldv;
    for (int c = tid; c < g.r; c += 256) g.G[(long long)p * g.ldg + c] = vecp[g.a + c];
  }
}

// the block columns before J0 of the tile rows from J0 on: rows move up, columns stay
__global__ __launch_bounds__(256) void k_rm_copy(RemoveArgs g) {
  const int tid = threadIdx.x, p = blockIdx.y, ps = g.slot[p];
  const int I = g.J0 + (int)blockIdx.x / g.J0, J = (int)blockIdx.x % g.J0;
  const double* __restrict__ As = g.A + (long long)ps * g.strideA;
  double* __restrict__ dst = g.ws + (long long)p * g.ws_stride + (tile_off(I, J) - g.off0);
  for (int idx = tid; idx < NB2; idx += 256) {
    const int col = idx >> 7, i = I * NB + (idx & 127);
    double v = 0.0;
    if (i < g.n_new) {
      const int oi = i < g.a ? i : i + g.r;
      v = As[tile_off(oi >> 7, J) + (long long)col * NB + (oi & 127)];
    }
    dst[idx] = v;
  }
}

__global__ __launch_bounds__(256) void k_rm_commit(RemoveArgs g) {
  const int p = blockIdx.y, ps = g.slot[p];
  const double* __restrict__ src = g.ws + (long long)p * g.ws_stride;
  double* __restrict__ dst = g.A + (long long)ps * g.strideA + g.off0;
  for (long long k = ((long long)blockIdx.x * 256 + threadIdx.x) * 2; k < g.ws_stride; k += (long long)gridDim.x * 512)
    *reinterpret_cast<d2*>(dst + k) = *reinterpret_cast<const d2*>(src + k);
}

// Diagonal tile (J, J): rows 0..127 of the tile are owned by lane pairs 0..127, the alpha row by pair 128 (wave 4).
template <int RH>
__global__ __launch_bounds__(320) void k_rm_panel(RemoveArgs g) {
  constexpr int RC = 2 * RH;
  __shared__ double sS[(NB + 1) * RM_LDS];
  __shared__ double sV[RM_CW * RC];
  __shared__ double sTau[NB], sDiag[NB], sAl[NB];
  __shared__ int sBad;
  const int tid = threadIdx.x, p = blockIdx.x, ps = g.slot[p], J = g.J;
  const int il = tid >> 1, h = tid & 1;
  const double* __restrict__ As = g.A + (long long)ps * g.strideA;
  double* __restrict__ wsp = g.ws + (long long)p * g.ws_stride;
  const double* __restrict__ Wkp = g.Wk + (long long)p * RM_RMAX * g.ldw;
  double* __restrict__ vecp = g.vec + (long long)ps * g.ldv;
  double* __restrict__ Vp = g.V + (long long)p * RM_VSTRIDE;
  double w[RH];
#pragma unroll
  for (int q = 0; q < RH; ++q) {
    const int c = h * RH + q;
    w[q] = 0.0;
    if (c < g.rc) {
      if (il < NB) w[q] = Wkp[(long long)c * g.ldw + J * NB + il];
      else if (il == NB) w[q] = g.G[(long long)p * g.ldg + g.c0 + c];
    }
  }
  if (tid == 0) sBad = 0;
  if (tid < NB) {
    const int gj = J * NB + tid;
    sAl[tid] = gj < g.n_new ? vecp[g.first ? (gj < g.a ? gj : gj + g.r) : gj] : 0.0;
  }
  __syncthreads();
  for (int cc = 0; cc < NB / RM_CW; ++cc) {
    for (int idx = tid; idx < NB * RM_CW; idx += 320) {
      const int col = idx >> 7, row = idx & 127;
      const int gi = J * NB + row, gj = J * NB + cc * RM_CW + col;
      double v = gi == gj ? 1.0 : 0.0;               // identity padding from n_new on; zeros above the diagonal
      if (gi >= gj && gi < g.n_new) v = rm_src(g, As, wsp, gi, gj);
      sS[row * RM_LDS + col] = v;
    }
    if (tid < RM_CW) sS[NB * RM_LDS + tid] = sAl[cc * RM_CW + tid];
    __syncthreads();
    for (int jl = 0; jl < RM_CW; ++jl) {
      const int j = cc * RM_CW + jl;
      if (il == j) {
        double xn = 0.0;
#pragma unroll
        for (int q = 0; q < RH; ++q) xn = fma(w[q], w[q], xn);
        xn += __shfl_xor(xn, 1);
        const double al = sS[j * RM_LDS + jl];
        double beta = al, tau = 0.0, sc = 0.0;
        if (xn > al * al * RM_NEGLIGIBLE) {
          beta = sqrt(fma(al, al, xn));
          const double apb = al + beta;
          tau = xn / (apb * beta);
          sc = -apb / xn;
        }
#pragma unroll
        for (int q = 0; q < RH; ++q) sV[jl * RC + h * RH + q] = w[q] * sc;
        if (h == 0) {
          sTau[j] = tau; sDiag[j] = beta; sS[j * RM_LDS + jl] = beta;
          if (!(beta > 0.0 && beta < 1.0e300) && sBad == 0) sBad = J * NB + j + 1;
        }
      }
      __syncthreads();
      const double tau = sTau[j];
      if (tau != 0.0 && il > j && il <= NB) {
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < RH; ++q) d = fma(w[q], sV[jl * RC + h * RH + q], d);
        d += __shfl_xor(d, 1);
        const double s0 = sS[il * RM_LDS + jl];
        const double ts = tau * (s0 + d);
#pragma unroll
        for (int q = 0; q < RH; ++q) w[q] = fma(-ts, sV[jl * RC + h * RH + q], w[q]);
        if (h == 0) sS[il * RM_LDS + jl] = s0 - ts;
      }
    }
    __syncthreads();
    double* __restrict__ dst = wsp + (tile_off(J, J) - g.off0) + (long long)cc * RM_CW * NB;
    for (int idx = tid; idx < NB * RM_CW; idx += 320) {
      const int col = idx >> 7, row = idx & 127;
      dst[idx] = row >= cc * RM_CW + col ? sS[row * RM_LDS + col] : 0.0;
    }
    for (int idx = tid; idx < RM_CW * RC; idx += 320) Vp[cc * RM_CW * RC + idx] = sV[idx];
    if (tid < RM_CW) {
      Vp[NB * RM_RMAX + cc * RM_CW + tid] = sTau[cc * RM_CW + tid];
      sAl[cc * RM_CW + tid] = sS[NB * RM_LDS + tid];
    }
    if (g.last && tid < RM_CW) {
      // inverses of the chunk's two 16 x 16 pivot blocks, column k by forward substitution; column-major like every 16 x 16 block
      const int bl = tid >> 4, k = tid & 15, b0 = cc * RM_CW + bl * 16;
      const double* Lb = sS + b0 * RM_LDS + bl * 16;
      double x[16];
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        double s = m == k ? -1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < m; ++q) s = fma(Lb[m * RM_LDS + q], x[q], s);
        x[m] = m < k ? 0.0 : -s / Lb[m * RM_LDS + m];
      }
      double* __restrict__ Wg = g.Winv + (((long long)ps * g.wsteps + J) * NSB + cc * 2 + bl) * 256;
#pragma unroll
      for (int m = 0; m < 16; ++m) Wg[k * 16 + m] = x[m];
    }
    __syncthreads();
  }
  if (il == NB) {
#pragma unroll
    for (int q = 0; q < RH; ++q) {
      const int c = h * RH + q;
      if (c < g.rc) g.G[(long long)p * g.ldg + g.c0 + c] = w[q];
    }
  }
  if (tid < NB) vecp[J * NB + tid] = sAl[tid];
  if (tid < 64) {
    double ss = sAl[tid] * sAl[tid] + sAl[tid + 64] * sAl[tid + 64];
    double ld = 2.0 * log(sDiag[tid]) + 2.0 * log(sDiag[tid + 64]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { ss += __shfl_xor(ss, off); ld += __shfl_xor(ld, off); }
    if (tid == 0) {
      double* pp = g.partial + ((long long)ps * g.ntp + J) * 2;
      pp[0] = ld;
      pp[1] = ss;
      if (sBad != 0 && g.info[ps] == 0) g.info[ps] = sBad;
    }
  }
}

// Tile (I, J), I > J: every row takes the 128 reflectors of tile column J in turn.
template <int RH>
__global__ __launch_bounds__(256) void k_rm_apply(RemoveArgs g) {
  constexpr int RC = 2 * RH;
  __shared__ double sS[NB * RM_LDS];
  __shared__ double sV[RM_CW * RC];
  __shared__ double sTau[RM_CW];
  const int tid = threadIdx.x, p = blockIdx.y, ps = g.slot[p], J = g.J, I = J + 1 + blockIdx.x;
  const int il = tid >> 1, h = tid & 1;
  const double* __restrict__ As = g.A + (long long)ps * g.strideA;
  double* __restrict__ wsp = g.ws + (long long)p * g.ws_stride;
  double* __restrict__ Wkp = g.Wk + (long long)p * RM_RMAX * g.ldw;
  const double* __restrict__ Vp = g.V + (long long)p * RM_VSTRIDE;
  double w[RH];
#pragma unroll
  for (int q = 0; q < RH; ++q) {
    const int c = h * RH + q;
    w[q] = c < g.rc ? Wkp[(long long)c * g.ldw + I * NB + il] : 0.0;
  }
  for (int cc = 0; cc < NB / RM_CW; ++cc) {
    for (int idx = tid; idx < NB * RM_CW; idx += 256) {
      const int col = idx >> 7, row = idx & 127;
      const int gi = I * NB + row, gj = J * NB + cc * RM_CW + col;
      sS[row * RM_LDS + col] = gi < g.n_new ? rm_src(g, As, wsp, gi, gj) : 0.0;
    }
    for (int idx = tid; idx < RM_CW * RC; idx += 256) sV[idx] = Vp[cc * RM_CW * RC + idx];
    if (tid < RM_CW) sTau[tid] = Vp[NB * RM_RMAX + cc * RM_CW + tid];
    __syncthreads();
    for (int jl = 0; jl < RM_CW; ++jl) {
      const double tau = sTau[jl];
      if (tau != 0.0) {
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < RH; ++q) d = fma(w[q], sV[jl * RC + h * RH + q], d);
        d += __shfl_xor(d, 1);
        const double s0 = sS[il * RM_LDS + jl];
        const double ts = tau * (s0 + d);
#pragma unroll
        for (int q = 0; q < RH; ++q) w[q] = fma(-ts, sV[jl * RC + h * RH + q], w[q]);
        if (h == 0) sS[il * RM_LDS + jl] = s0 - ts;
      }
    }
    __syncthreads();
    double* __restrict__ dst = wsp + (tile_off(I, J) - g.off0) + (long long)cc * RM_CW * NB;
    for (int idx = tid; idx < NB * RM_CW; idx += 256) dst[idx] = sS[(idx & 127) * RM_LDS + (idx >> 7)];
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < RH; ++q) {
    const int c = h * RH + q;
    if (c < g.rc) Wkp[(long long)c * g.ldw + I * NB + il] = w[q];
  }
}

}  // namespace agp
