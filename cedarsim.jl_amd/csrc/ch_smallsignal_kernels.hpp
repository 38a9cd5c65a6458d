// ch_smallsignal_kernels.hpp — device side of the small-signal family (AC, noise, DC and AC parameter sensitivities): the dense
// solvers ac_block_kernel, sens_block_kernel and acsens_solve_kernel, the right-hand-side and state-shift kernels of ch_ac_sens, the
// noise table, and their argument structs.  Included by ch_kernels.hpp inside namespace chip, at the spot where this text stood:
// the order in which the kernels are emitted into the code object is part of the measured build (profiles/r07_notes.md section 4).
#pragma once

// ---------------------------------------------------------------------------------------------
// Small-signal frequency sweep: (G + jωC) x = b per (block, sample, frequency) — ac! / freqresp
// (src/ac.jl:75-102, 267-284) and, transposed with a unit right-hand side, the adjoint solve behind
// noise! / PSD (src/ac.jl:136-163, 286-305).  G, C and b come from MODE_EVAL dumps of the Newton kernel
// at the DC operating point, so the device arithmetic is the one the transient uses.
// One wavefront per (frequency, block): complex dense LU with partial pivoting (ch_dense_lu.hpp) in LDS; one 256-thread workgroup
// with a global workspace for coupled systems that do not fit LDS.
struct AcArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C; const double* b;  // dumps: [nblk][ds][ds], [nblk][ds]
  int ds, S, n_unk, n_freq, n_comp;
  const double* omega;                                // [n_freq] rad/s
  double* x_out;                                      // AC: [S][n_freq][n_unk][2]
  // noise (adjoint) mode
  int noise, comp_out, row_out;                       // block and block-local row of the output unknown
  int n_noise;                                        // entries of the noise table per sample (unused entries: pwr = 0)
  const int* noise_a; const int* noise_b;             // [S][n_noise] block-local unknown of each terminal or -1 (known node)
  const double* noise_pwr; const double* noise_exp;   // [S][n_noise] power at the operating point, flicker exponent (0 = white)
  double* psd_out;                                    // [S][n_freq]
  int* fail;                                          // set to 1 when a factorisation breaks down
  double* work; int f0;                               // global workspace [systems of this launch][2*nc*(nc+1)] (T = 256 variant); first frequency of this launch
  double* contrib_out; const int* contrib_col; int n_col;   // CONTRIB instantiations: [S][n_freq][n_col], the share of the PSD of every table entry that owns a column (contrib_col[n_noise]: its column, or -1)
};

// T = 64: one wavefront, matrices in LDS (blocks of the fused path, coupled systems up to 96 unknowns).
// T = 256: one workgroup, matrices in a global workspace (a.work; larger coupled systems of the sparse path) — same algorithm,
// workgroup barriers instead of wave-local fences.
// CONTRIB (noise mode with a contributions buffer, ch_noise_ex): beside the sum, the |y_a - y_b|^2 pwr / f^ex of every table entry that owns a column is
// stored — what ngspice prints per device under .noise.  The instantiations without it are the code they were.
template <int T, bool CONTRIB = false>
__global__ __launch_bounds__(T) void ac_block_kernel(const AcArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = a.f0 + blockIdx.x;
  const int blk = a.noise ? a.comp_out * a.S + (int)blockIdx.y : (int)blockIdx.y;
  const int c = blk / a.S, s = blk - c * a.S;
  const BlockMeta bm = a.bmeta[c];
  const int nc = bm.cm.nc, lda = nc + 1;
  double* Ar = a.work ? a.work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 2 * (size_t)nc * lda : lds;
  double* Ai = Ar + (size_t)nc * lda;
  const double w = a.omega[f];
  const double* G = a.G + (long)blk * a.ds * a.ds; const double* Cg = a.C + (long)blk * a.ds * a.ds;
  for (int e = tid; e < nc * nc; e += T) {
    const int r = e / nc, col = e - r * nc;
    const int src = a.noise ? col * nc + r : e;  // adjoint: transpose
    Ar[r * lda + col] = G[src]; Ai[r * lda + col] = w * Cg[src];
  }
  for (int i = tid; i < nc; i += T) { Ar[i * lda + nc] = a.noise ? (i == a.row_out ? 1.0 : 0.0) : a.b[(long)blk * a.ds + i]; Ai[i * lda + nc] = 0.0; }
  lu_fence<T>();
  // the augmented form of the family's LU (ch_dense_lu.hpp): the right-hand side is eliminated with its rows, so only U x = y is left
  const bool ok = clu_factor<T>(Ar, Ai, nullptr, nc, lda, 1, s_best, s_bi);
  if (ok) clu_back_column<T>(Ar, Ai, Ar + nc, Ai + nc, nc, lda, lda);
  else if (tid == 0) *a.fail = 1;
  if (!a.noise) {
    double* xo = a.x_out + (((long)s * a.n_freq + f) * a.n_unk + bm.uofs) * 2;
    for (int i = tid; i < nc; i += T) { xo[2 * i] = ok ? Ar[i * lda + nc] : CH_NAN; xo[2 * i + 1] = ok ? Ai[i * lda + nc] : CH_NAN; }
  } else {
    // output PSD = Σ_k |y_a - y_b|² · pwr_k / f^exp_k  (PSD(dss, ωs, pwr, exp), src/ac.jl:286-298)
    const double fhz = w * 0.15915494309189535;
    double acc = 0.0;
    for (int k = tid; k < a.n_noise; k += T) {
      const long e = (long)s * a.n_noise + k;
      const double pw = a.noise_pwr[e];
      int cc = -1;
      if constexpr (CONTRIB) { cc = a.contrib_col[k]; if (cc >= 0 && (pw == 0.0 || !ok)) a.contrib_out[((long)s * a.n_freq + f) * a.n_col + cc] = ok ? 0.0 : CH_NAN; }
      if (pw == 0.0) continue;
      const int na = a.noise_a[e], nb = a.noise_b[e];
      const double yr = (na >= 0 ? Ar[na * lda + nc] : 0.0) - (nb >= 0 ? Ar[nb * lda + nc] : 0.0);
      const double yi = (na >= 0 ? Ai[na * lda + nc] : 0.0) - (nb >= 0 ? Ai[nb * lda + nc] : 0.0);
      const double ex = a.noise_exp[e];
      if constexpr (CONTRIB) {
        const double term = (yr * yr + yi * yi) * (ex == 0.0 ? pw : pw / pow(fhz, ex));
        if (ok && cc >= 0) a.contrib_out[((long)s * a.n_freq + f) * a.n_col + cc] = term;
        acc += term;
      } else acc += (yr * yr + yi * yi) * (ex == 0.0 ? pw : pw / pow(fhz, ex));
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
    if (tid == 0) a.psd_out[(long)s * a.n_freq + f] = ok ? acc : CH_NAN;
  }
}

// ---------------------------------------------------------------------------------------------
// DC parameter sensitivities, direct method (ch_dc_sens): G · dx/dp_k = -dF/dp_k per (block, sample), G from the same MODE_EVAL dump
// the small-signal analyses use and dF/dp_k from two residual evaluations at the fixed operating point.  The real
// dense LU of the family (rlu_solve, ch_dense_lu.hpp) over the augmented matrix [G | b_0 … b_{kc-1}]: elimination and back
// substitution over all kc right-hand sides at once.  The arithmetic of a column does not depend on which other columns share the
// launch, so chunks of parameters give the bits one launch would.
struct SensArgs {
  const BlockMeta* bmeta;
  const double* G;                       // [nblk][ds][ds]
  const double* Fp; const double* Fm;    // first column of this launch: [kc][nblk][ds], f_stride doubles per column
  const double* den;                     // [kc][S]: F+ - F- is divided by this (2h central, h forward)
  const int* skip;                       // [S] != 0: the sample's operating point failed, nothing is solved or written
  long f_stride;
  int ds, S, n_unk, n_par, k0, kc, blk0;
  double* x_out;                         // [S][n_par][n_unk], unknown order
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work;                          // T = 256: global workspace [blocks of this launch][nc * lda]
};

// T = 64: one wavefront, [G | B] in LDS with the odd row stride lda = (nc + kc) | 1 — a walk down a column (pivot search, multipliers)
// then reads 32 different bank pairs per half-wave, and the row updates are contiguous.  T = 256: one workgroup, global workspace.
template <int T>
__global__ __launch_bounds__(T) void sens_block_kernel(const SensArgs a) {
  extern __shared__ double lds[];
  __shared__ double s_best[4]; __shared__ int s_bi[4];
  const int tid = threadIdx.x;
  const int blk = a.blk0 + (int)blockIdx.x, c = blk / a.S, s = blk - c * a.S;
  if (a.skip[s]) return;
  const BlockMeta bm = a.bmeta[c];
  const int nc = bm.cm.nc, kc = a.kc, lda = (nc + kc) | 1;
  double* A = a.work ? a.work + (size_t)blockIdx.x * nc * lda : lds;
  const double* G = a.G + (long)blk * a.ds * a.ds;
  for (int e = tid; e < nc * nc; e += T) { const int r = e / nc, col = e - r * nc; A[r * lda + col] = G[e]; }
  for (int e = tid; e < nc * kc; e += T) {
    const int j = e / nc, i = e - j * nc;
    const long f = (long)j * a.f_stride + (long)blk * a.ds + i;
    A[i * lda + nc + j] = -(a.Fp[f] - a.Fm[f]) / a.den[(long)j * a.S + s];
  }
  lu_fence<T>();
  const bool ok = rlu_solve<T>(A, nc, kc, lda, s_best, s_bi);
  if (!ok && tid == 0) *a.fail = 1;
  for (int e = tid; e < nc * kc; e += T) {
    const int j = e / nc, i = e - j * nc;
    a.x_out[((long)s * a.n_par + a.k0 + j) * a.n_unk + bm.uofs + i] = ok ? A[i * lda + nc + j] : CH_NAN;
  }
}

// ---------------------------------------------------------------------------------------------
// AC parameter sensitivities, direct method (ch_ac_sens): Y dx/dp_k = -(dY/dp_k) x with Y = G + jwC, x the ordinary ac_block_kernel
// solution and dY/dp_k = dG + jw dC a difference of two MODE_EVAL dumps (the explicit term: perturbed tables at the fixed operating
// point; the state term: the circuit's tables at x* +- eps s_k).  acsens_rhs_kernel accumulates one such contribution into the
// right-hand sides of one parameter, acsens_solve_kernel factors Y once per (frequency, block, sample) and solves all parameters.
struct AcSensRhsArgs {
  const BlockMeta* bmeta;
  const double* Gp; const double* Gm; const double* Cp; const double* Cm;   // dumps [nblk][ds][ds] of the two evaluations
  const double* den;                     // [S]: the differences are divided by this
  const int* skip;                       // [S] != 0: nothing is read or written for the sample
  const double* x;                       // [S][n_freq][n_unk][2]
  const double* omega;                   // [n_freq]
  double* R;                             // this parameter's right-hand sides [nblk][n_freq][ds][2], accumulated into
  int ds, S, n_unk, n_freq;
};

// One workgroup per (block, sample, tile of ACSENS_FT frequencies); a wavefront owns a row of the difference matrix, its lanes walk
// the row (the contiguous axis of the dump, and of x) and keep one complex partial sum per frequency of the tile, so the matrices are
// read once per tile.  The partial sums of a frequency do not depend on its tile companions, and the wave reduction is a fixed tree.
constexpr int ACSENS_FT = 8;
__global__ __launch_bounds__(256) void acsens_rhs_kernel(const AcSensRhsArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int blk = blockIdx.x, c = blk / a.S, s = blk - c * a.S;
  if (a.skip[s]) return;
  const BlockMeta bm = a.bmeta[c];
  const int nc = bm.cm.nc, f0 = (int)blockIdx.y * ACSENS_FT, nf = min(ACSENS_FT, a.n_freq - f0);
  const double den = a.den[s];
  const long mofs = (long)blk * a.ds * a.ds;
  const double* x = a.x + (((long)s * a.n_freq + f0) * a.n_unk + bm.uofs) * 2;
  double w[ACSENS_FT];
#pragma unroll
  for (int q = 0; q < ACSENS_FT; ++q) w[q] = q < nf ? a.omega[f0 + q] : 0.0;
  for (int i = wv; i < nc; i += 4) {
    double ar[ACSENS_FT], ai[ACSENS_FT];
#pragma unroll
    for (int q = 0; q < ACSENS_FT; ++q) { ar[q] = 0.0; ai[q] = 0.0; }
    for (int j = lane; j < nc; j += 64) {
      const long e = mofs + (long)i * nc + j;
      const double dg = (a.Gp[e] - a.Gm[e]) / den, dc = (a.Cp[e] - a.Cm[e]) / den;
      if (dg == 0.0 && dc == 0.0) continue;
#pragma unroll
      for (int q = 0; q < ACSENS_FT; ++q) {
        if (q >= nf) break;
        const double xr = x[((long)q * a.n_unk + j) * 2], xi = x[((long)q * a.n_unk + j) * 2 + 1], wc = w[q] * dc;
        ar[q] += dg * xr - wc * xi; ai[q] += dg * xi + wc * xr;
      }
    }
#pragma unroll
    for (int q = 0; q < ACSENS_FT; ++q) { ar[q] = wave_sum(ar[q]); ai[q] = wave_sum(ai[q]); }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < ACSENS_FT; ++q) {
        if (q >= nf) break;
        double* r = a.R + (((long)blk * a.n_freq + f0 + q) * a.ds + i) * 2;
        r[0] -= ar[q]; r[1] -= ai[q];
      }
    }
  }
}

// the state of the state term: X[dst] = X[0] + sign * eps[s] * s_k per sample (eps = 0: the operating point itself)
__global__ void acsens_shift_kernel(double* X, long slot_stride, int dst, const double* sx, int k, int n_par, const double* eps, double sign, int n_unk, int S) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)S * n_unk) return;
  const int s = (int)(i / n_unk), u = (int)(i - (long)s * n_unk);
  const double e = eps[s];
  X[(long)dst * slot_stride + i] = e != 0.0 ? X[i] + sign * e * sx[((long)s * n_par + k) * n_unk + u] : X[i];
}

struct AcSensSolveArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C;      // [nblk][ds][ds]
  const double* R;                       // [n_par][nblk][n_freq][ds][2]
  const double* omega;                   // [n_freq]
  const int* skip;                       // [S] != 0: the sample's operating point failed, nothing is solved or written
  int ds, S, n_unk, n_freq, n_par, nblk, kp, f0;   // kp: columns of a panel; f0: first frequency of this launch
  double* x_out;                         // [S][n_freq][n_par][n_unk][2], unknown order
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work; long work_per;           // T = 256: global workspace, work_per doubles per system of this launch
};

// The in-place form of the family's complex LU (clu_factor with `perm`, clu_substitute of ch_dense_lu.hpp) on Y(w), written out
// here: on the shared templates the 64-thread instantiation was 0.9 % slower than it had been (ch_ac_sens, 96 unknowns; DESIGN.md
// 2.7j), so this kernel keeps its own text.  Then the n_par right-hand sides in panels of kp columns: gather through the
// permutation, forward and back substitution over all columns of the panel at once.  A column's arithmetic never reads another column, so any panelling gives the same bits.
// T = 64: one wavefront, factors and panel in LDS, odd row stride lda = nc | 1 for the column walks.  T = 256: one workgroup, the
// same layout in a global workspace.
template <int T>
__global__ __launch_bounds__(T) void acsens_solve_kernel(const AcSensSolveArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4]; __shared__ int s_perm[MULTI ? 1 : 96];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = a.f0 + blockIdx.x;
  const int blk = blockIdx.y, c = blk / a.S, s = blk - c * a.S;
  if (a.skip[s]) return;
  const BlockMeta bm = a.bmeta[c];
  const int nc = bm.cm.nc, lda = nc | 1, kp = a.kp;
  double* Ar = MULTI ? a.work + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)a.work_per : lds;
  double* Ai = Ar + (size_t)nc * lda;
  double* Br = Ai + (size_t)nc * lda;
  double* Bi = Br + (size_t)nc * kp;
  int* perm = MULTI ? (int*)(Bi + (size_t)nc * kp) : s_perm;
  auto fence = [&]() { if (MULTI) __syncthreads(); else wave_fence(); };
  const double w = a.omega[f];
  const double* G = a.G + (long)blk * a.ds * a.ds; const double* Cg = a.C + (long)blk * a.ds * a.ds;
  for (int e = tid; e < nc * nc; e += T) { const int r = e / nc, col = e - r * nc; Ar[r * lda + col] = G[e]; Ai[r * lda + col] = w * Cg[e]; }
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
    for (int e = tid; e < nc * a.n_par; e += T) {
      const int j = e / nc, i = e - j * nc;
      double* xo = a.x_out + (((((long)s * a.n_freq + f) * a.n_par + j) * a.n_unk) + bm.uofs + i) * 2;
      xo[0] = CH_NAN; xo[1] = CH_NAN;
    }
    return;
  }
  for (int k0 = 0; k0 < a.n_par; k0 += kp) {
    const int kc = min(kp, a.n_par - k0);
    for (int e = tid; e < nc * kc; e += T) {
      const int j = e / nc, i = e - j * nc;
      const double* r = a.R + ((((long)(k0 + j) * a.nblk + blk) * a.n_freq + f) * a.ds + perm[i]) * 2;
      Br[i * kp + j] = r[0]; Bi[i * kp + j] = r[1];
    }
    fence();
    for (int k = 0; k < nc - 1; ++k) {   // L y = P b
      const int rem = nc - k - 1;
      for (int e = tid; e < rem * kc; e += T) {
        const int i = k + 1 + e / kc, j = e % kc;
        const double lr = Ar[i * lda + k], li = Ai[i * lda + k], br = Br[k * kp + j], bi_ = Bi[k * kp + j];
        Br[i * kp + j] -= lr * br - li * bi_; Bi[i * kp + j] -= lr * bi_ + li * br;
      }
      fence();
    }
    for (int k = nc - 1; k >= 0; --k) {   // U x = y
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
    for (int e = tid; e < nc * kc; e += T) {
      const int j = e / nc, i = e - j * nc;
      double* xo = a.x_out + (((((long)s * a.n_freq + f) * a.n_par + k0 + j) * a.n_unk) + bm.uofs + i) * 2;
      xo[0] = Br[i * kp + j]; xo[1] = Bi[i * kp + j];
    }
    fence();
  }
}

// Noise sources of the output block at the DC operating point (slot `x_slot` of the state ring): resistors
// (white_noise(dscope, 4kT/res, :thermal), src/simpledevices.jl:72-76) and the white/flicker sources of compiled
// Verilog-A modules.  One thread per (device of the block, sample); every device owns va::MAX_NOISE table entries.
struct NoiseTabArgs {
  const int* dkind; const int* dterm; const int* dsrc; const int* dcls_local; const int* dhdev;
  const double* dpar; const double* dmult; const double* vapar; long va_stride; const double* temp_s; const double* gmin_s;
  const double* X; const double* kv;   // state (slot already applied) [S][n_unk]; known-node values [Ssrc][nk]
  int Spar, Stemp, Sgmin, Ssrc, nk, S, n_unk, dofs, ndev, uofs, nc;
  int* na; int* nb; double* pwr; double* ex;
};
__global__ void noise_table_kernel(const NoiseTabArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.ndev * a.S) return;
  const int dl = i % a.ndev, s = i / a.ndev, d = a.dofs + dl;
  const long base = ((long)s * a.ndev + dl) * va::MAX_NOISE;
  for (int k = 0; k < va::MAX_NOISE; ++k) { a.na[base + k] = -1; a.nb[base + k] = -1; a.pwr[base + k] = 0.0; a.ex[base + k] = 0.0; }
  const int kind = a.dkind[d];
  const int* tm = a.dterm + NTERM * d;
  auto loc = [&](int t) { return (t >= a.uofs && t < a.uofs + a.nc) ? t - a.uofs : -1; };
  const long pi = (long)a.dhdev[d] * a.Spar + (a.Spar > 1 ? s : 0);
  const double T = a.temp_s[a.Stemp > 1 ? s : 0] + 273.15;
  if (kind == K_R) {
    a.na[base] = loc(tm[0]); a.nb[base] = loc(tm[1]);
    a.pwr[base] = 4.0 * 1.380649e-23 * T * a.dmult[pi] / a.dpar[pi];
  } else if (kind == K_VA) {
    double vv[NTERM];
    for (int k = 0; k < NTERM; ++k) { const int t = tm[k]; vv[k] = t >= 0 ? a.X[(long)s * a.n_unk + t] : a.kv[(long)(a.Ssrc > 1 ? s : 0) * a.nk + (-t - 1)]; }
    va::NoiseRec rec[va::MAX_NOISE];
    const va::Env env{T, a.gmin_s[a.Sgmin > 1 ? s : 0]};
    const int n = va_gen::noise(a.dcls_local[d], a.vapar + (long)s * a.va_stride + a.dsrc[d], vv, env, rec);
    for (int k = 0; k < n && k < va::MAX_NOISE; ++k) {
      a.na[base + k] = rec[k].a >= 0 ? loc(tm[rec[k].a]) : -1;
      a.nb[base + k] = rec[k].b >= 0 ? loc(tm[rec[k].b]) : -1;
      a.pwr[base + k] = a.dmult[pi] * rec[k].pwr; a.ex[base + k] = rec[k].ex;
    }
  }
}

// Noise sources of the BSIM4 MOSFETs of the output block (ch_noise_ex with mos_noise): the second launch behind noise_table_kernel
// on the same stream, which has zeroed the entries this kernel fills.  One thread per (device of the block, sample); a thread
// whose device is no MOSFET leaves.  Terminal voltages from the state slot and the known-node values as for K_VA above; b4_noise
// (ch_bsim4.hpp) forms the mode frame, so a device whose drain and source are exchanged keeps its source between the same two
// nodes; the noise parameters come from their own table, one row per MOSFET class (ch_noise_params.hpp), uploaded for this
// analysis alone.  Entry 0: channel thermal noise, entry 1: flicker noise (ch_b4_noise.hpp), both drain to source, times m.
struct MosNoiseArgs {
  const int* dkind; const int* dterm; const int* dhdev; const int* dcls;
  const double* dmult; const double* temp_s; const double* mosp; const double* npar;   // npar: [MOS classes][CH_B4N_NPAR]
  const double* X; const double* kv;   // as in NoiseTabArgs
  int Spar, Stemp, Ssrc, Smos, nk, S, n_unk, dofs, ndev, uofs, nc;
  int* na; int* nb; double* pwr; double* ex;
  double* operands;                    // [S][ndev][B4NO_COUNT] or null: the operand rows, for diagnosis and the parity tests
  int* fail;                           // set to 1 when a card has no intrinsic charge model to take qinv from
};
__global__ void mos_noise_table_kernel(const MosNoiseArgs a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.ndev * a.S) return;
  const int dl = i % a.ndev, s = i / a.ndev, d = a.dofs + dl;
  if (a.dkind[d] != K_MOS) {
    if (a.operands) for (int k = 0; k < B4NO_COUNT; ++k) a.operands[((long)s * a.ndev + dl) * B4NO_COUNT + k] = 0.0;
    return;
  }
  const long base = ((long)s * a.ndev + dl) * va::MAX_NOISE;
  const int* tm = a.dterm + NTERM * d;
  auto loc = [&](int t) { return (t >= a.uofs && t < a.uofs + a.nc) ? t - a.uofs : -1; };
  double vv[4];
  for (int k = 0; k < 4; ++k) { const int t = tm[k]; vv[k] = t >= 0 ? a.X[(long)s * a.n_unk + t] : a.kv[(long)(a.Ssrc > 1 ? s : 0) * a.nk + (-t - 1)]; }
  const int cl = a.dcls[d];
  const B4Col P = b4_col(a.mosp, (long)cl * a.Smos + (a.Smos > 1 ? s : 0));
  double op[B4NO_COUNT];
  if (!b4_noise(P, vv[0], vv[1], vv[2], vv[3], op)) *a.fail = 1;
  B4NoiseRec rec[2];
  const double T = a.temp_s[a.Stemp > 1 ? s : 0] + 273.15;
  const int n = b4_noise_records(op, a.npar + (long)cl * CH_B4N_NPAR, T, rec);
  const double m = a.dmult[(long)a.dhdev[d] * a.Spar + (a.Spar > 1 ? s : 0)];
  for (int k = 0; k < n; ++k) {
    a.na[base + k] = loc(tm[rec[k].a]); a.nb[base + k] = loc(tm[rec[k].b]);
    a.pwr[base + k] = m * rec[k].pwr; a.ex[base + k] = rec[k].ex;
  }
  if (a.operands) for (int k = 0; k < B4NO_COUNT; ++k) a.operands[((long)s * a.ndev + dl) * B4NO_COUNT + k] = op[k];
}
