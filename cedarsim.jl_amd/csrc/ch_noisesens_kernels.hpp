// ch_noisesens_kernels.hpp — device side of the noise PSD parameter sensitivities (ch_noise_sens), direct method on the adjoint
// system.  With Y = G + jwC and Y^T y = e_out the PSD is S = sum_e |dy_e|^2 pwr_e / f^ex_e, dy_e = y[a_e] - y[b_e]; for a slot p_k
//   Y^T dy_k = -(dY/dp_k)^T y,    dS/dp_k = sum_e [ 2 Re(conj(dy_e) d(dy)_{k,e}) pwr_e + |dy_e|^2 dpwr_{k,e} ] / f^ex_e.
// noisesens_rhs_kernel accumulates one difference of G, C dumps into the right-hand sides of one parameter, noisesens_dpwr_kernel
// one difference of source tables into its dpwr, and noisesens_solve_kernel factors Y^T once per (frequency, sample) of the
// output block, solves y and every parameter column and reduces over the table.  Included by ch_engine.hip behind
// ch_measure_kernels.hpp: the kernels in front of it keep their place in the code object (their emission order is part of the
// measured build, ch_smallsignal_kernels.hpp).
#pragma once

namespace chip {

struct NoiseSensRhsArgs {
  const BlockMeta* bmeta;
  const double* Gp; const double* Gm; const double* Cp; const double* Cm;   // dumps [nblk][ds][ds] of the two evaluations
  const double* den;                     // [S]: the differences are divided by this
  const int* skip;                       // [S] != 0: nothing is read or written for the sample
  const double* y;                       // [S][n_freq][nc][2]: the adjoint solution of the output block
  const double* omega;                   // [n_freq]
  double* R;                             // this parameter's right-hand sides [S][n_freq][ds][2], accumulated into
  int ds, S, n_freq, comp;               // comp: the output block
};

// The transposed sibling of acsens_rhs_kernel: R[f][j] -= sum_i (dG[i][j] + jw_f dC[i][j]) y[f][i].  One wavefront per (sample, tile
// of ACSENS_FT frequencies, 64 columns); a lane owns a column j — the contiguous axis of the dumps, so a row of the difference is one
// coalesced load — and walks the rows in order with one complex partial sum per frequency of the tile in registers: the matrices
// are read once per tile, y[f][i] is the same address in every lane, and a zero difference skips its y loads.  The sum of a
// frequency is a fixed sequence of its own terms: no atomics, no dependence on the tile companions.
__global__ __launch_bounds__(64) void noisesens_rhs_kernel(const NoiseSensRhsArgs a) {
  const int s = blockIdx.x;
  if (a.skip[s]) return;
  const int nc = a.bmeta[a.comp].cm.nc, j = (int)blockIdx.z * 64 + (int)threadIdx.x;
  if (j >= nc) return;
  const int f0 = (int)blockIdx.y * ACSENS_FT, nf = min(ACSENS_FT, a.n_freq - f0);
  const double den = a.den[s];
  const long mofs = ((long)a.comp * a.S + s) * a.ds * a.ds;
  const double* y = a.y + ((long)s * a.n_freq + f0) * nc * 2;
  double w[ACSENS_FT], ar[ACSENS_FT], ai[ACSENS_FT];
#pragma unroll
  for (int q = 0; q < ACSENS_FT; ++q) { w[q] = q < nf ? a.omega[f0 + q] : 0.0; ar[q] = 0.0; ai[q] = 0.0; }
  for (int i = 0; i < nc; ++i) {
    const long e = mofs + (long)i * nc + j;
    const double dg = (a.Gp[e] - a.Gm[e]) / den, dc = (a.Cp[e] - a.Cm[e]) / den;
    if (dg == 0.0 && dc == 0.0) continue;
#pragma unroll
    for (int q = 0; q < ACSENS_FT; ++q) {
      if (q >= nf) break;
      const double yr = y[((long)q * nc + i) * 2], yi = y[((long)q * nc + i) * 2 + 1], wc = w[q] * dc;
      ar[q] += dg * yr - wc * yi; ai[q] += dg * yi + wc * yr;
    }
  }
#pragma unroll
  for (int q = 0; q < ACSENS_FT; ++q) {
    if (q >= nf) break;
    double* r = a.R + (((long)s * a.n_freq + f0 + q) * a.ds + j) * 2;
    r[0] -= ar[q]; r[1] -= ai[q];
  }
}

// dpwr[s][e] += (pwr+ - pwr-) / den[s] for the entries of the output block's source table, one thread per entry.  The exponent of
// an entry is not differentiated: a table whose ex differs from the operating point's raises the flag.
struct NoiseSensDpwrArgs {
  const double* pwr_p; const double* pwr_m; const double* ex_p; const double* ex_m; const double* ex0;   // [S][n_tab]
  const double* den;                     // [S]
  const int* skip;                       // [S]
  double* dpwr;                          // this parameter's [S][n_tab], accumulated into
  int* ex_moved;                         // this parameter's flag
  int S, n_tab;
};
__global__ void noisesens_dpwr_kernel(const NoiseSensDpwrArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.S * a.n_tab) return;
  const int s = (int)(i / a.n_tab);
  if (a.skip[s]) return;
  if (a.ex_p[i] != a.ex0[i] || a.ex_m[i] != a.ex0[i]) *a.ex_moved = 1;
  a.dpwr[i] += (a.pwr_p[i] - a.pwr_m[i]) / a.den[s];
}

struct NoiseSensSolveArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C;      // [nblk][ds][ds]
  const double* R;                       // [n_par][S][n_freq][ds][2]
  const double* omega;                   // [n_freq]
  const int* skip;                       // [S] != 0: the sample's operating point failed, nothing is solved or written
  int ds, S, n_freq, n_par, kp, f0;      // kp: columns of a panel; f0: first frequency of this launch
  int comp, row_out, n_tab;              // output block, block-local row of the output unknown, entries of the source table per sample
  const int* na; const int* nb;          // [S][n_tab]: block-local unknown of each terminal or -1
  const double* pwr; const double* ex;   // [S][n_tab]: the table at the operating point
  const double* dpwr;                    // [n_par][S][n_tab]
  double* y_out;                         // n_par == 0: [S][n_freq][nc][2]
  double* dpsd_out;                      // n_par > 0: [S][n_freq][n_par]
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work; long work_per;           // T = 256: global workspace, work_per doubles per system of this launch
};

// The in-place complex LU of ch_dense_lu.hpp (clu_factor with `perm`, clu_substitute) on the transposed system, written out here: on
// the shared templates the 256-thread instantiation gave other bits in dpsd (noise_chunks of tests/test_gpu_sens_driver_bits.py, 302
// unknowns) with the same instruction mix, so this kernel keeps its own text.  Complex LU of Y^T(w) with partial
// pivoting (magnitude |re| + |im|, lowest row on ties) kept in place — multipliers below the diagonal, the row permutation in
// `perm` — then the unit column for y, which stays resident, then the n_par right-hand sides in panels of kp columns: gather
// through the permutation, forward and back substitution over all columns of the panel at once, and per column the reduction over
// the table entries.  A column's arithmetic never reads another column, so any panelling gives the same bits.  n_par == 0: y is
// stored and nothing else.
// T = 64: one wavefront, factors, y and panel in LDS, odd row stride lda = nc | 1 for the column walks.  T = 256: one workgroup, the
// same layout in a global workspace.
template <int T>
__global__ __launch_bounds__(T) void noisesens_solve_kernel(const NoiseSensSolveArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4]; __shared__ int s_perm[MULTI ? 1 : 96];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = a.f0 + blockIdx.x;
  const int s = blockIdx.y, blk = a.comp * a.S + s;
  if (a.skip[s]) return;
  const int nc = a.bmeta[a.comp].cm.nc, lda = nc | 1, kp = a.kp;
  double* Ar = MULTI ? a.work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)a.work_per : lds;
  double* Ai = Ar + (size_t)nc * lda;
  double* Yr = Ai + (size_t)nc * lda;
  double* Yi = Yr + nc;
  double* Br = Yi + nc;
  double* Bi = Br + (size_t)nc * kp;
  int* perm = MULTI ? (int*)(Bi + (size_t)nc * kp) : s_perm;
  auto fence = [&]() { if (MULTI) __syncthreads(); else wave_fence(); };
  const double w = a.omega[f];
  const double* G = a.G + (long)blk * a.ds * a.ds; const double* Cg = a.C + (long)blk * a.ds * a.ds;
  for (int e = tid; e < nc * nc; e += T) { const int r = e / nc, col = e - r * nc; Ar[col * lda + r] = G[e]; Ai[col * lda + r] = w * Cg[e]; }   // transposed
  for (int i = tid; i < nc; i += T) perm[i] = i;
  fence();
  bool ok = true;
  for (int k = 0; k < nc; ++k) {
    double best = -1.0; int bi = k;
    for (int i = k + tid; i < nc; i += T) { const double v = fabs(Ar[i * lda + k]) + fabs(Ai[i * lda + k]); if (v > best) { best = v; bi = i; } }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (MULTI) {
      if (lane == 0) { s_best[wv] = best; s_bi[wv] = bi; }
      __syncthreads();
      best = s_best[0]; bi = s_bi[0];
#pragma unroll
      for (int q = 1; q < T / 64; ++q) { const double ob = s_best[q]; const int oi = s_bi[q]; if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; } }
      __syncthreads();   // s_best / s_bi are rewritten in the next step
    }
    if (!(best > 0.0) || !(best < 1e300)) { ok = false; break; }
    if (bi != k) {   // whole rows: the multipliers already stored move with their row
      for (int j = tid; j < nc; j += T) {
        double t = Ar[k * lda + j]; Ar[k * lda + j] = Ar[bi * lda + j]; Ar[bi * lda + j] = t;
        t = Ai[k * lda + j]; Ai[k * lda + j] = Ai[bi * lda + j]; Ai[bi * lda + j] = t;
      }
      if (tid == 0) { const int t = perm[k]; perm[k] = perm[bi]; perm[bi] = t; }
      fence();
    }
    const double pr = Ar[k * lda + k], pi = Ai[k * lda + k];
    const double den = 1.0 / (pr * pr + pi * pi), ir = pr * den, ii = -pi * den;  // 1/pivot
    for (int i = k + 1 + tid; i < nc; i += T) {
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k];
      Ar[i * lda + k] = lr * ir - li * ii; Ai[i * lda + k] = lr * ii + li * ir;
    }
    fence();
    const int rem = nc - k - 1;
    for (int e = tid; e < rem * rem; e += T) {
      const int i = k + 1 + e / rem, j = k + 1 + e % rem;
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k], ur = Ar[k * lda + j], ui = Ai[k * lda + j];
      Ar[i * lda + j] -= lr * ur - li * ui; Ai[i * lda + j] -= lr * ui + li * ur;
    }
    fence();
  }
  if (!ok) {   // (`ok` is uniform over the workgroup: every thread holds the reduced pivot)
    if (tid == 0) *a.fail = 1;
    if (a.n_par == 0) for (int i = tid; i < 2 * nc; i += T) a.y_out[((long)s * a.n_freq + f) * nc * 2 + i] = CH_NAN;
    for (int j = tid; j < a.n_par; j += T) a.dpsd_out[((long)s * a.n_freq + f) * a.n_par + j] = CH_NAN;
    return;
  }
  // ---- y: L U y = P e_out ----
  for (int i = tid; i < nc; i += T) { Yr[i] = perm[i] == a.row_out ? 1.0 : 0.0; Yi[i] = 0.0; }
  fence();
  for (int k = 0; k < nc - 1; ++k) {
    const double br = Yr[k], bi_ = Yi[k];
    for (int i = k + 1 + tid; i < nc; i += T) {
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k];
      Yr[i] -= lr * br - li * bi_; Yi[i] -= lr * bi_ + li * br;
    }
    fence();
  }
  for (int k = nc - 1; k >= 0; --k) {
    const double pr = Ar[k * lda + k], pi = Ai[k * lda + k], br = Yr[k], bi_ = Yi[k];
    const double den = 1.0 / (pr * pr + pi * pi);
    const double xr = (br * pr + bi_ * pi) * den, xi = (bi_ * pr - br * pi) * den;
    fence();
    if (tid == 0) { Yr[k] = xr; Yi[k] = xi; }
    for (int i = tid; i < k; i += T) {
      const double ur = Ar[i * lda + k], ui = Ai[i * lda + k];
      Yr[i] -= ur * xr - ui * xi; Yi[i] -= ur * xi + ui * xr;
    }
    fence();
  }
  if (a.n_par == 0) {
    double* yo = a.y_out + ((long)s * a.n_freq + f) * nc * 2;
    for (int i = tid; i < nc; i += T) { yo[2 * i] = Yr[i]; yo[2 * i + 1] = Yi[i]; }
    return;
  }
  const double fhz = w * 0.15915494309189535;
  for (int k0 = 0; k0 < a.n_par; k0 += kp) {
    const int kc = min(kp, a.n_par - k0);
    for (int e = tid; e < nc * kc; e += T) {
      const int j = e / nc, i = e - j * nc;
      const double* r = a.R + ((((long)(k0 + j) * a.S + s) * a.n_freq + f) * a.ds + perm[i]) * 2;
      Br[i * kp + j] = r[0]; Bi[i * kp + j] = r[1];
    }
    fence();
    for (int k = 0; k < nc - 1; ++k) {   // L z = P b
      const int rem = nc - k - 1;
      for (int e = tid; e < rem * kc; e += T) {
        const int i = k + 1 + e / kc, j = e % kc;
        const double lr = Ar[i * lda + k], li = Ai[i * lda + k], br = Br[k * kp + j], bi_ = Bi[k * kp + j];
        Br[i * kp + j] -= lr * br - li * bi_; Bi[i * kp + j] -= lr * bi_ + li * br;
      }
      fence();
    }
    for (int k = nc - 1; k >= 0; --k) {   // U dy = z
      const double pr = Ar[k * lda + k], pi = Ai[k * lda + k], den = 1.0 / (pr * pr + pi * pi);
      for (int j = tid; j < kc; j += T) {
        const double br = Br[k * kp + j], bi_ = Bi[k * kp + j];
        Br[k * kp + j] = (br * pr + bi_ * pi) * den; Bi[k * kp + j] = (bi_ * pr - br * pi) * den;
      }
      fence();
      for (int e = tid; e < k * kc; e += T) {
        const int i = e / kc, j = e - i * kc;
        const double ur = Ar[i * lda + k], ui = Ai[i * lda + k], xr = Br[k * kp + j], xi = Bi[k * kp + j];
        Br[i * kp + j] -= ur * xr - ui * xi; Bi[i * kp + j] -= ur * xi + ui * xr;
      }
      fence();
    }
    // dS/dp_k = sum_e [ 2 Re(conj(dy_e) d(dy)_e) pwr_e + |dy_e|^2 dpwr_e ] / f^ex_e, a column at a time
    for (int j = 0; j < kc; ++j) {
      const double* dpw = a.dpwr + ((long)(k0 + j) * a.S + s) * a.n_tab;
      double acc = 0.0;
      for (int e = tid; e < a.n_tab; e += T) {
        const long te = (long)s * a.n_tab + e;
        const double pw = a.pwr[te], dp = dpw[e];
        if (pw == 0.0 && dp == 0.0) continue;
        const int na = a.na[te], nb = a.nb[te];
        const double yr = (na >= 0 ? Yr[na] : 0.0) - (nb >= 0 ? Yr[nb] : 0.0), yi = (na >= 0 ? Yi[na] : 0.0) - (nb >= 0 ? Yi[nb] : 0.0);
        const double zr = (na >= 0 ? Br[na * kp + j] : 0.0) - (nb >= 0 ? Br[nb * kp + j] : 0.0);
        const double zi = (na >= 0 ? Bi[na * kp + j] : 0.0) - (nb >= 0 ? Bi[nb * kp + j] : 0.0);
        const double v = 2.0 * (yr * zr + yi * zi) * pw + (yr * yr + yi * yi) * dp, ex = a.ex[te];
        acc += ex == 0.0 ? v : v / pow(fhz, ex);
      }
      acc = wave_sum(acc);
      if (MULTI) {
        __syncthreads();
        if (lane == 0) s_best[wv] = acc;
        __syncthreads();
        acc = 0.0;
#pragma unroll
        for (int q = 0; q < T / 64; ++q) acc += s_best[q];
      }
      if (tid == 0) a.dpsd_out[((long)s * a.n_freq + f) * a.n_par + k0 + j] = acc;
    }
    fence();
  }
}

}  // namespace chip
