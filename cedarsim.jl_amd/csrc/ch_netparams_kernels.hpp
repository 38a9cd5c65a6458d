// ch_netparams_kernels.hpp — device side of the N-port network analysis (ch_net_params).  With Y = G + jwC at the operating point and
// P voltage-source ports (ch_netparams_host.hpp):
//   Y x_k = b_k (port k at 1 V, the others AC shorts),   Yp[j][k] = -x_k[row_i(j)],   Y^T l_j = e_row_i(j),
//   dYp[j][k]/dp = l_j^T (dY/dp) x_k,   S, Z, dS, dZ by the P x P conversions of the host header.
// netparams_solve_kernel factors Y once per (frequency, sample) of the ports' block and solves the P excitations; when parameters
// are asked for it factors Y^T as well and solves the P unit columns.  netparams_bilinear_kernel adds the P^2 bilinear forms of one
// difference of G, C dumps into dYp of one parameter, netparams_convert_kernel turns Yp, dYp into the S and Z rows.  Included behind
// ch_loopgain_kernels.hpp, the last device header of ch_engine.hip: the kernels in front keep their place in the code object.
#pragma once

#include "ch_netparams_host.hpp"

namespace chip {

struct NetParamsSolveArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C;      // [nblk][ds][ds]
  const double* b;                       // ac_rhs's vector [nblk][ds]: the sum of the P excitations
  const double* omega;                   // [n_freq]
  const int* skip;                       // [S] != 0: the sample's operating point failed, NaN is written
  const int* rows;                       // [P]: block-local row of every port's branch current
  int ds, S, n_freq, f0;                 // f0: first frequency of this launch
  int comp, P;                           // the ports' block, the number of ports
  int adjoint;                           // != 0: the P solutions and the P adjoint vectors are stored as well
  double* Yp;                            // [P*P][n_freq][S][2]
  double* vec;                           // [2P][S][n_freq][nc][2]: x_0 .. x_{P-1}, l_0 .. l_{P-1}
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work; long work_per;           // T = 256: global workspace, work_per doubles per system of this launch
};

// The P-column sibling of loopgain_solve_kernel: the in-place form of the family's complex LU (clu_factor with `perm`,
// clu_substitute, ch_dense_lu.hpp), one system per (frequency, sample), the ports' block alone.
// T = 64: one wavefront, factors and the P-column panel in LDS (up to 96 unknowns).  T = 256: one workgroup, the same layout in a
// global workspace.  Pass 0 factors Y and solves the P columns b_k (the entry of b in port k's branch row, alone); with a.adjoint,
// pass 1 factors Y^T (the transposed load of the same dumps) and solves the P unit columns.
template <int T>
__global__ __launch_bounds__(T) void netparams_solve_kernel(const NetParamsSolveArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4]; __shared__ int s_perm[MULTI ? 1 : 96];
  const int tid = threadIdx.x, f = a.f0 + blockIdx.x, s = blockIdx.y, blk = a.comp * a.S + s, P = a.P;
  const long fs = (long)f * a.S + s, row_ld = (long)a.n_freq * a.S;
  const int nc = a.bmeta[a.comp].cm.nc, lda = nc | 1;
  if (a.skip && a.skip[s]) {
    for (int e = tid; e < P * P; e += T) { double* y = a.Yp + (e * row_ld + fs) * 2; y[0] = CH_NAN; y[1] = CH_NAN; }
    return;
  }
  double* Ar = MULTI ? a.work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)a.work_per : lds;
  double* Ai = Ar + (size_t)nc * lda;
  double* Br = Ai + (size_t)nc * lda;
  double* Bi = Br + (size_t)nc * P;
  int* perm = MULTI ? (int*)(Bi + (size_t)nc * P) : s_perm;
  const double w = a.omega[f];
  const double* G = a.G + (long)blk * a.ds * a.ds; const double* Cg = a.C + (long)blk * a.ds * a.ds;
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
    for (int e = tid; e < nc * P; e += T) {
      const int i = e / P, k = e - i * P, p = perm[i];
      Br[e] = p == a.rows[k] ? (pass == 0 ? a.b[(long)blk * a.ds + p] : 1.0) : 0.0;
      Bi[e] = 0.0;
    }
    lu_fence<T>();
    clu_substitute<T>(Ar, Ai, Br, Bi, nc, lda, P, P);
    if (pass == 0) {
      for (int e = tid; e < P * P; e += T) {   // Yp[j][k] = -x_k[row_i(j)]
        const int j = e / P, k = e - j * P, at = a.rows[j] * P + k;
        double* y = a.Yp + (e * row_ld + fs) * 2;
        y[0] = -Br[at]; y[1] = -Bi[at];
      }
    }
    if (a.adjoint) {
      for (int e = tid; e < nc * P; e += T) {
        const int i = e / P, k = e - i * P;
        double* v = a.vec + ((((long)(P * pass + k) * a.S + s) * a.n_freq + f) * nc + i) * 2;
        v[0] = Br[e]; v[1] = Bi[e];
      }
    }
    lu_fence<T>();   // the next pass overwrites the panel
  }
  if (!ok) {
    if (tid == 0) *a.fail = 1;
    for (int e = tid; e < P * P; e += T) { double* y = a.Yp + (e * row_ld + fs) * 2; y[0] = CH_NAN; y[1] = CH_NAN; }
    if (a.adjoint) for (int e = tid; e < 2 * P * nc; e += T) {
      double* v = a.vec + ((((long)(e / nc) * a.S + s) * a.n_freq + f) * nc + e % nc) * 2;
      v[0] = CH_NAN; v[1] = CH_NAN;
    }
  }
}

struct NetParamsBilinearArgs {
  const BlockMeta* bmeta;
  const double* Gp; const double* Gm; const double* Cp; const double* Cm;   // dumps [nblk][ds][ds] of the two evaluations
  const double* den;                     // [S]: the differences are divided by this
  const int* skip;                       // [S] != 0: nothing is read or written for the sample
  const double* vec;                     // [2P][S][n_freq][nc][2]: x_0 .. x_{P-1}, l_0 .. l_{P-1}
  const double* omega;                   // [n_freq]
  double* dY;                            // this parameter's dYp: entry r = j * P + k at dY + r * row_ld * 2, [n_freq][S][2] each, accumulated into
  long row_ld;                           // doubles / 2 between two entries' rows: n_par * n_freq * S
  int ds, S, n_freq, comp, P;
};

// dYp[j][k][f] += l_j^T D x_k with D = (G+ - G-)/den + jw_f (C+ - C-)/den, for all k of one adjoint port j = blockIdx.z.  One
// workgroup per (sample, tile of NET_FT frequencies, j); a wavefront owns rows of D, its lanes walk the row (the contiguous axis of
// the dumps and of the x_k) and keep P complex partial sums per frequency of the tile in registers (the loops over the tile and the
// ports are unrolled to CH_NET_MAX_PORTS: no indexed private array), so D is read once per tile and a zero entry skips its loads.
// The wave reduction is a fixed tree and the four wave sums are added in wave order: a frequency's sum does not depend on its tile
// companions, nor on the other parameters of the call (one launch per difference of one parameter).
constexpr int NET_FT = 2;
__global__ __launch_bounds__(256) void netparams_bilinear_kernel(const NetParamsBilinearArgs a) {
  __shared__ double red[4][NET_FT][CH_NET_MAX_PORTS][2];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, s = blockIdx.x, jp = blockIdx.z, P = a.P;
  if (a.skip[s]) return;
  const int nc = a.bmeta[a.comp].cm.nc, f0 = (int)blockIdx.y * NET_FT, nf = min(NET_FT, a.n_freq - f0);
  const double den = a.den[s];
  const long mofs = ((long)a.comp * a.S + s) * a.ds * a.ds, plane = (long)a.S * a.n_freq * nc * 2;
  const double* x0 = a.vec + ((long)s * a.n_freq + f0) * nc * 2;
  const double* lj = x0 + (long)(P + jp) * plane;
  double w[NET_FT], ar[NET_FT][CH_NET_MAX_PORTS], ai[NET_FT][CH_NET_MAX_PORTS];
#pragma unroll
  for (int q = 0; q < NET_FT; ++q) {
    w[q] = q < nf ? a.omega[f0 + q] : 0.0;
#pragma unroll
    for (int k = 0; k < CH_NET_MAX_PORTS; ++k) { ar[q][k] = 0.0; ai[q][k] = 0.0; }
  }
  for (int i = wv; i < nc; i += 4) {
    for (int j = lane; j < nc; j += 64) {
      const long e = mofs + (long)i * nc + j;
      const double dg = (a.Gp[e] - a.Gm[e]) / den, dc = (a.Cp[e] - a.Cm[e]) / den;
      if (dg == 0.0 && dc == 0.0) continue;
#pragma unroll
      for (int q = 0; q < NET_FT; ++q) {
        if (q >= nf) break;
        const long ri = ((long)q * nc + i) * 2, cj = ((long)q * nc + j) * 2;
        const double wc = w[q] * dc;
        const double tr = lj[ri] * dg - lj[ri + 1] * wc, ti = lj[ri] * wc + lj[ri + 1] * dg;   // l_j[i] * D[i][j]
#pragma unroll
        for (int k = 0; k < CH_NET_MAX_PORTS; ++k) {
          if (k >= P) break;
          const double xr = x0[k * plane + cj], xi = x0[k * plane + cj + 1];
          ar[q][k] += tr * xr - ti * xi; ai[q][k] += tr * xi + ti * xr;
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NET_FT; ++q) {
#pragma unroll
    for (int k = 0; k < CH_NET_MAX_PORTS; ++k) {
      if (k >= P) break;
      const double sr = wave_sum(ar[q][k]), si = wave_sum(ai[q][k]);
      if (lane == 0) { red[wv][q][k][0] = sr; red[wv][q][k][1] = si; }
    }
  }
  __syncthreads();
  if (tid < nf * P * 2) {
    const int q = tid / (2 * P), k = (tid >> 1) % P, c = tid & 1;
    const double sum = ((red[0][q][k][c] + red[1][q][k][c]) + red[2][q][k][c]) + red[3][q][k][c];
    a.dY[((long)(jp * P + k) * a.row_ld + (long)(f0 + q) * a.S + s) * 2 + c] += sum;
  }
}

struct NetParamsConvertArgs {
  const double* Yp; const double* dYp;   // [P*P][n_freq][S][2], [P*P][n_par][n_freq][S][2] (null without parameters)
  double* Sm; double* dSm;               // the S rows and their derivative rows, or null: nobody asked
  double* Zm; double* dZm;               // the Z rows and their derivative rows, or null
  double* work;                          // [P*P][n_freq * S][2]
  const double* rz;                      // [P]: sqrt(z0)
  const int* skip;                       // [S] != 0: NaN rows
  long n_fs; int S, P, n_par;
};

// One thread per (frequency, sample): Yp -> S, Z and dYp -> dS, dZ of every parameter by the host header's conversions, on the rows
// where they lie (an entry's element stride is a row: n_freq * S, or n_par * n_freq * S).  A breakdown of Yp leaves NaN in Z and dZ
// of this (frequency, sample) alone, one of I + y in S and dS; neither is a failure of the analysis.
__global__ __launch_bounds__(64) void netparams_convert_kernel(const NetParamsConvertArgs a) {
  const long fs = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (fs >= a.n_fs) return;
  const int P = a.P, s = (int)(fs % a.S);
  const long dld = (long)a.n_par * a.n_fs;
  NetCMat Y; Y.p = a.Yp + fs * 2; Y.st = a.n_fs;
  NetMat W; W.p = a.work + fs * 2; W.st = a.n_fs;
  const bool skip = a.skip[s] != 0;
  for (int kind = 0; kind < 2; ++kind) {
    double* V = kind == 0 ? a.Sm : a.Zm; double* dV = kind == 0 ? a.dSm : a.dZm;
    if (!V) continue;
    NetMat M; M.p = V + fs * 2; M.st = a.n_fs;
    bool ok = !skip;
    if (skip) net_fill_nan(M, P);
    else ok = kind == 0 ? net_y_to_s(Y, a.rz, W, M, P) : net_y_to_z(Y, W, M, P);
    if (!dV) continue;
    for (int k = 0; k < a.n_par; ++k) {
      NetMat dM; dM.p = dV + ((long)k * a.n_fs + fs) * 2; dM.st = dld;
      NetCMat dY; dY.p = a.dYp + ((long)k * a.n_fs + fs) * 2; dY.st = dld;
      if (!ok) net_fill_nan(dM, P);
      else if (kind == 0) net_dy_to_ds(net_const(M), dY, a.rz, W, dM, P);
      else net_dy_to_dz(net_const(M), dY, W, dM, P);
    }
  }
}

}  // namespace chip
