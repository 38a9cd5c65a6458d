// ch_transens_kernels.hpp — device side of the transient parameter sensitivities (ch_tran_sens): transens_step_kernel, one step of
// the s / w recursion of ch_transens_host.hpp per (block, sample) for a chunk of parameters, and save_sens_kernel, the saved rows.
// Included by ch_engine.hip behind every other device header: the kernels in front of it keep their place in the code object.
#pragma once

namespace chip {

// (G + a0 C) s_k = -[ (f+ - f-)/den_k + a0 (q+ - q-)/den_k + sum_j a_j W[hist_j][k] ],   W[cand][k] = C s_k + (q+ - q-)/den_k
// per (block, sample), G, C, f, q from MODE_EVAL dumps at the accepted state (a0 = 0, no history in them).  The real dense
// LU of sens_block_kernel (rlu_solve, ch_dense_lu.hpp) over [G + a0 C | b_0 .. b_{kc-1}], written out here: on the shared template
// the solve launches of the 100-slot ladder were 3.6 % slower than they had been, so this kernel keeps its own
// text.  Elimination and back substitution over all columns at once.  A column's arithmetic never reads another column, so chunks of
// parameters give the bits one launch would.
struct TranSensArgs {
  const BlockMeta* bmeta;
  const double* G; const double* C;      // [nblk][ds][ds]
  const double* F0; const double* Q0;    // [nblk][ds]: the unperturbed evaluation, the minus side of a forward difference
  const double* Fp; const double* Fm; const double* Qp; const double* Qm;   // [n_par][nblk][ds], f_stride doubles per parameter
  const double* den;                     // [n_par][S]: the differences are divided by this (2h central, h forward)
  const int* central;                    // [n_par] != 0: the minus side is Fm / Qm, else F0 / Q0
  double* Sr; double* Wr;                // rings [NSLOT][n_par][S][n_unk]
  double alpha[6]; int hist_slot[5];     // the accepted step's BDF coefficients and history slots (alpha[0] = 0, k = 0: a DC solve)
  int k, cand;                           // order; the ring slot written
  int solve;                             // 0: s is read from Sr[cand] (the start of a transient), only W[cand] is formed
  long f_stride;
  int ds, S, n_unk, n_par, k0, kc, blk0;
  int* fail;                             // set to 1 when a factorisation breaks down
  double* work;                          // T = 256: global workspace [blocks of this launch][nc * lda]
};

// T = 64: one wavefront, [A | B] in LDS with the odd row stride lda = (nc + kc) | 1 (column walks of the pivot search and the
// multipliers touch every bank once); C streams from the global dump in the epilogue.  T = 256: one workgroup, global workspace.
template <int T>
__global__ __launch_bounds__(T) void transens_step_kernel(const TranSensArgs a) {
  extern __shared__ double lds[];
  constexpr bool MULTI = T > 64;
  __shared__ double s_best[4]; __shared__ int s_bi[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int blk = a.blk0 + (int)blockIdx.x, c = blk / a.S, s = blk - c * a.S;
  const BlockMeta bm = a.bmeta[c];
  const int nc = bm.cm.nc, kc = a.kc, lda = (nc + kc) | 1;
  double* A = a.work ? a.work + (size_t)blockIdx.x * nc * lda : lds;
  auto fence = [&]() { if (MULTI) __syncthreads(); else wave_fence(); };
  const double a0 = a.alpha[0];
  const long mofs = (long)blk * a.ds * a.ds, vofs = (long)blk * a.ds;
  auto ring = [&](int slot, int j, int i) { return (((long)slot * a.n_par + a.k0 + j) * a.S + s) * a.n_unk + bm.uofs + i; };
  // (q+ - q-)/den of column j, row i: needed by the right-hand side and again by W
  auto dq_of = [&](int j, int i) {
    const long f = (long)(a.k0 + j) * a.f_stride + vofs + i;
    return (a.Qp[f] - (a.central[a.k0 + j] ? a.Qm[f] : a.Q0[vofs + i])) / a.den[(long)(a.k0 + j) * a.S + s];
  };
  bool ok = true;
  if (a.solve) {
    for (int e = tid; e < nc * nc; e += T) { const int r = e / nc, col = e - r * nc; A[r * lda + col] = a.G[mofs + e] + a0 * a.C[mofs + e]; }
    for (int e = tid; e < nc * kc; e += T) {
      const int j = e / nc, i = e - j * nc;
      const long f = (long)(a.k0 + j) * a.f_stride + vofs + i;
      const double df = (a.Fp[f] - (a.central[a.k0 + j] ? a.Fm[f] : a.F0[vofs + i])) / a.den[(long)(a.k0 + j) * a.S + s];
      double h = 0.0;
      for (int m = 1; m <= a.k; ++m) h += a.alpha[m] * a.Wr[ring(a.hist_slot[m - 1], j, i)];
      A[i * lda + nc + j] = -(df + a0 * dq_of(j, i) + h);
    }
    fence();
    for (int k = 0; k < nc && ok; ++k) {
      double best = -1.0; int bi = k;
      for (int i = k + tid; i < nc; i += T) { const double v = fabs(A[i * lda + k]); if (v > best) { best = v; bi = i; } }
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
      if (bi != k) {
        for (int j = k + tid; j < nc + kc; j += T) { const double t = A[k * lda + j]; A[k * lda + j] = A[bi * lda + j]; A[bi * lda + j] = t; }
        fence();
      }
      const double piv = A[k * lda + k];
      for (int i = k + 1 + tid; i < nc; i += T) A[i * lda + k] /= piv;
      fence();
      const int rem = nc - k - 1, wd = rem + kc;
      for (int e = tid; e < rem * wd; e += T) {
        const int i = k + 1 + e / wd, j = k + 1 + e % wd;
        A[i * lda + j] -= A[i * lda + k] * A[k * lda + j];
      }
      fence();
    }
    if (ok) {
      for (int k = nc - 1; k >= 0; --k) {
        const double piv = A[k * lda + k];
        for (int j = tid; j < kc; j += T) A[k * lda + nc + j] /= piv;
        fence();
        for (int e = tid; e < k * kc; e += T) {
          const int i = e / kc, j = e - i * kc;
          A[i * lda + nc + j] -= A[i * lda + k] * A[k * lda + nc + j];
        }
        fence();
      }
    } else if (tid == 0) *a.fail = 1;
  } else {
    for (int e = tid; e < nc * kc; e += T) { const int i = e / kc, j = e - i * kc; A[i * lda + nc + j] = a.Sr[ring(a.cand, j, i)]; }
    fence();
  }
  // epilogue: S[cand][k] = s_k, W[cand][k] = C s_k + dq_k.  The lanes of a row share its C entries (one broadcast load each) and
  // read neighbouring columns of the solution in LDS
  for (int e = tid; e < nc * kc; e += T) {
    const int i = e / kc, j = e - i * kc;
    double w = 0.0;
    const double* Ci = a.C + mofs + (long)i * nc;
    for (int l = 0; l < nc; ++l) w += Ci[l] * A[l * lda + nc + j];
    const long o = ring(a.cand, j, i);
    if (a.solve) a.Sr[o] = ok ? A[i * lda + nc + j] : CH_NAN;
    a.Wr[o] = ok ? w + dq_of(j, i) : CH_NAN;
  }
}

// One saved row of sensitivities: the weighted sum of S ring slots the state row uses (save_obs_kernel), for every observable and
// parameter: dst[obs][par][sample].  An observable without an unknown (known node, eliminated branch) is filled in by the host.
struct SensObsArgs { const double* Sr; int slots[8]; double w[8]; int nw; int n_unk, S, n_obs, n_par; const int* obs_unk; double* dst; };
__global__ void save_sens_kernel(const SensObsArgs a) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)a.n_obs * a.n_par * a.S) return;
  const int s = (int)(i % a.S), k = (int)((i / a.S) % a.n_par), o = (int)(i / ((long)a.S * a.n_par));
  const int u = a.obs_unk[o];
  double v = 0.0;
  if (u >= 0) for (int j = 0; j < a.nw; ++j) v += a.w[j] * a.Sr[(((long)a.slots[j] * a.n_par + k) * a.S + s) * a.n_unk + u];
  a.dst[i] = v;
}

}  // namespace chip
