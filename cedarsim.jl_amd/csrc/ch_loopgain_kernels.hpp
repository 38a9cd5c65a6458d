// ch_loopgain_kernels.hpp — device side of the loop-gain (stability) analysis (ch_loop_gain).  With Y = G + jwC at the operating point
// and a voltage-source probe x -> y in the loop wire (ch_loopgain_host.hpp):
//   Y x_v = b_v (the probe at 1 V),   Y x_i = b_i (unit current into x),   u = x_v[x] - x_i[i_p],   T = u / (1 - u),
//   Y^T l_x = e_x,   Y^T l_i = e_ip,   du/dp_k = -l_x^T (dY/dp_k) x_v + l_i^T (dY/dp_k) x_i,   dT/dp_k = (du/dp_k) / (1 - u)^2.
// loopgain_solve_kernel factors Y once per (frequency, sample) of the probe's block and solves both excitations; when parameters
// are asked for it factors Y^T as well and solves the two unit columns.  loopgain_bilinear_kernel adds the two bilinear forms of one
// difference of G, C dumps into du of one parameter, loopgain_dt_kernel turns du into dT rows.  Included by ch_engine.hip behind every
// device header but ch_netparams_kernels.hpp: the kernels in front keep their place in the code object (their emission order is part of the measured
// build, ch_smallsignal_kernels.hpp).
#pragma once

#include "ch_loopgain_host.hpp"

namespace chip {

struct LoopGainSolveArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C;      // [nblk][ds][ds]
  const double* b;                       // ac_rhs's vector [nblk][ds]: b_v
  const double* omega;                   // [n_freq]
  const int* skip;                       // [S] != 0: the sample's operating point failed, NaN is written
  int ds, S, n_freq, f0;                 // f0: first frequency of this launch
  int comp, row_x, row_i;                // the probe's block; block-local rows of v_x (its KCL row takes b_i) and of the branch current
  int adjoint;                           // != 0: u, the two solutions and the two adjoint vectors are stored as well
  double bi;                             // the entry of b_i in row_x
  double* T_out;                         // [n_freq][S][2]
  double* u_out;                         // [n_freq][S][2]
  double* vec;                           // [4][S][n_freq][nc][2]: x_v, x_i, l_x, l_i
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work; long work_per;           // T = 256: global workspace, work_per doubles per system of this launch
};

// The in-place form of the family's complex LU (clu_factor with `perm`, clu_substitute, ch_dense_lu.hpp): one system per (frequency,
// sample), the probe's block alone.
// T = 64: one wavefront, factors and the two-column panel in LDS, odd row stride lda = nc | 1 for the column walks (up to 96
// unknowns).  T = 256: one workgroup, the same layout in a global workspace.  Pass 0 factors Y and solves [b_v | b_i]; with
// a.adjoint, pass 1 factors Y^T (a second factorisation: the transposed load of the same dumps) and solves [e_x | e_ip].
template <int T>
__global__ __launch_bounds__(T) void loopgain_solve_kernel(const LoopGainSolveArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4]; __shared__ int s_perm[MULTI ? 1 : 96];
  const int tid = threadIdx.x, f = a.f0 + blockIdx.x, s = blockIdx.y, blk = a.comp * a.S + s;
  const long fs = (long)f * a.S + s;
  const int nc = a.bmeta[a.comp].cm.nc, lda = nc | 1;
  if (a.skip && a.skip[s]) {
    if (tid == 0) { a.T_out[2 * fs] = CH_NAN; a.T_out[2 * fs + 1] = CH_NAN; if (a.adjoint) { a.u_out[2 * fs] = CH_NAN; a.u_out[2 * fs + 1] = CH_NAN; } }
    return;
  }
  double* Ar = MULTI ? a.work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)a.work_per : lds;
  double* Ai = Ar + (size_t)nc * lda;
  double* Br = Ai + (size_t)nc * lda;
  double* Bi = Br + (size_t)nc * 2;
  int* perm = MULTI ? (int*)(Bi + (size_t)nc * 2) : s_perm;
  const double w = a.omega[f];
  const double* G = a.G + (long)blk * a.ds * a.ds; const double* Cg = a.C + (long)blk * a.ds * a.ds;
  double ur = 0.0, ui = 0.0;
  bool ok = true;
  for (int pass = 0; pass < (a.adjoint ? 2 : 1); ++pass) {
    for (int e = tid; e < nc * nc; e += T) {
      const int r = e / nc, col = e - r * nc, at = pass == 0 ? r * lda + col : col * lda + r;   // pass 1: transposed
      Ar[at] = G[e]; Ai[at] = w * Cg[e];
    }
    for (int i = tid; i < nc; i += T) perm[i] = i;
    lu_fence<T>();
    ok = clu_factor<T>(Ar, Ai, perm, nc, lda, 0, s_best, s_bi);
    if (!ok) break;
    for (int i = tid; i < nc; i += T) {
      const int p = perm[i];
      Br[i * 2] = pass == 0 ? a.b[(long)blk * a.ds + p] : (p == a.row_x ? 1.0 : 0.0);
      Br[i * 2 + 1] = pass == 0 ? (p == a.row_x ? a.bi : 0.0) : (p == a.row_i ? 1.0 : 0.0);
      Bi[i * 2] = 0.0; Bi[i * 2 + 1] = 0.0;
    }
    lu_fence<T>();
    clu_substitute<T>(Ar, Ai, Br, Bi, nc, lda, 2, 2);
    if (pass == 0) { ur = Br[a.row_x * 2] - Br[a.row_i * 2 + 1]; ui = Bi[a.row_x * 2] - Bi[a.row_i * 2 + 1]; }   // u = V2 - I1
    if (a.adjoint) {
      for (int e = tid; e < nc * 2; e += T) {
        const int i = e >> 1, j = e & 1;
        double* v = a.vec + ((((long)(2 * pass + j) * a.S + s) * a.n_freq + f) * nc + i) * 2;
        v[0] = Br[e]; v[1] = Bi[e];
      }
    }
    lu_fence<T>();   // the next pass overwrites the panel
  }
  if (!ok) {
    if (tid == 0) *a.fail = 1;
    ur = CH_NAN; ui = CH_NAN;
    if (a.adjoint) for (int e = tid; e < 4 * nc; e += T) {
      double* v = a.vec + ((((long)(e / nc) * a.S + s) * a.n_freq + f) * nc + e % nc) * 2;
      v[0] = CH_NAN; v[1] = CH_NAN;
    }
  }
  if (tid == 0) {
    double tr = CH_NAN, ti = CH_NAN;
    if (ok) loopgain_T_of_u(ur, ui, tr, ti);
    a.T_out[2 * fs] = tr; a.T_out[2 * fs + 1] = ti;
    if (a.adjoint) { a.u_out[2 * fs] = ur; a.u_out[2 * fs + 1] = ui; }
  }
}

struct LoopGainBilinearArgs {
  const BlockMeta* bmeta;
  const double* Gp; const double* Gm; const double* Cp; const double* Cm;   // dumps [nblk][ds][ds] of the two evaluations
  const double* den;                     // [S]: the differences are divided by this
  const int* skip;                       // [S] != 0: nothing is read or written for the sample
  const double* vec;                     // [4][S][n_freq][nc][2]: x_v, x_i, l_x, l_i
  const double* omega;                   // [n_freq]
  double* du;                            // this parameter's [n_freq][S][2], accumulated into
  int ds, S, n_freq, comp;
};

// du[f] += -l_x^T D x_v + l_i^T D x_i with D = (G+ - G-)/den + jw_f (C+ - C-)/den.  One workgroup per (sample, tile of ACSENS_FT
// frequencies); a wavefront owns rows of D, its lanes walk the row (the contiguous axis of the dumps, and of x_v, x_i) and keep one
// complex partial sum per frequency of the tile, so D is read once per tile and a zero entry skips its loads.  The wave reduction
// is a fixed tree and the four wave sums are added in wave order: the sum of a frequency does not depend on its tile companions.
__global__ __launch_bounds__(256) void loopgain_bilinear_kernel(const LoopGainBilinearArgs a) {
  __shared__ double red[4][ACSENS_FT][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = blockIdx.x;
  if (a.skip[s]) return;
  const int nc = a.bmeta[a.comp].cm.nc, f0 = (int)blockIdx.y * ACSENS_FT, nf = min(ACSENS_FT, a.n_freq - f0);
  const double den = a.den[s];
  const long mofs = ((long)a.comp * a.S + s) * a.ds * a.ds, plane = (long)a.S * a.n_freq * nc * 2;
  const double* xv = a.vec + ((long)s * a.n_freq + f0) * nc * 2;
  const double* xi = xv + plane; const double* lx = xi + plane; const double* li = lx + plane;
  double w[ACSENS_FT], ar[ACSENS_FT], ai[ACSENS_FT];
#pragma unroll
  for (int q = 0; q < ACSENS_FT; ++q) { w[q] = q < nf ? a.omega[f0 + q] : 0.0; ar[q] = 0.0; ai[q] = 0.0; }
  for (int i = wv; i < nc; i += 4) {
    for (int j = lane; j < nc; j += 64) {
      const long e = mofs + (long)i * nc + j;
      const double dg = (a.Gp[e] - a.Gm[e]) / den, dc = (a.Cp[e] - a.Cm[e]) / den;
      if (dg == 0.0 && dc == 0.0) continue;
#pragma unroll
      for (int q = 0; q < ACSENS_FT; ++q) {
        if (q >= nf) break;
        const long ri = ((long)q * nc + i) * 2, cj = ((long)q * nc + j) * 2;
        const double wc = w[q] * dc;
        const double pr = dg * xv[cj] - wc * xv[cj + 1], pi = dg * xv[cj + 1] + wc * xv[cj];   // (D x_v)'s term
        const double qr = dg * xi[cj] - wc * xi[cj + 1], qi = dg * xi[cj + 1] + wc * xi[cj];   // (D x_i)'s term
        ar[q] += (li[ri] * qr - li[ri + 1] * qi) - (lx[ri] * pr - lx[ri + 1] * pi);
        ai[q] += (li[ri] * qi + li[ri + 1] * qr) - (lx[ri] * pi + lx[ri + 1] * pr);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < ACSENS_FT; ++q) { ar[q] = wave_sum(ar[q]); ai[q] = wave_sum(ai[q]); }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < ACSENS_FT; ++q) { red[wv][q][0] = ar[q]; red[wv][q][1] = ai[q]; }
  }
  __syncthreads();
  if (tid < 2 * nf) {
    const int q = tid >> 1, c = tid & 1;
    const double sum = ((red[0][q][c] + red[1][q][c]) + red[2][q][c]) + red[3][q][c];
    a.du[((long)(f0 + q) * a.S + s) * 2 + c] += sum;
  }
}

// dT[k][f][s] = du[k][f][s] / (1 - u[f][s])^2: the rows the measure kernels read (FRows.dH, ldS = S).  One thread per (f, s) and parameter.
__global__ __launch_bounds__(256) void loopgain_dt_kernel(const double* u, const double* du, double* dT, long n_fs, int n_par) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_fs * n_par) return;
  const long fs = i % n_fs;
  double dr, di;
  loopgain_dT_of_du(u[2 * fs], u[2 * fs + 1], du[2 * i], du[2 * i + 1], dr, di);
  dT[2 * i] = dr; dT[2 * i + 1] = di;
}

}  // namespace chip
