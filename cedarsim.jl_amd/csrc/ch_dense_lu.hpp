// ch_dense_lu.hpp — the dense LU with partial pivoting of the small-signal and sensitivity kernels: ac_block_kernel,
// sens_block_kernel (ch_smallsignal_kernels.hpp) and loopgain_solve_kernel.  acsens_solve_kernel, noisesens_solve_kernel and
// transens_step_kernel hold the same steps written out: on these templates the first and the last ran slower than they had, and the
// bits of the second moved.  Forced-inline device templates only, no kernel: nothing here is emitted or callable on its own.  T is the workgroup size: 64, one wavefront on LDS with
// wave-local fences, or 256, one workgroup on a global workspace with barriers.
// Every matrix element is updated by one thread with one expression, so a kernel's bits do not depend on T's partner or on which
// other right-hand sides share its panel.  Included by ch_kernels.hpp inside namespace chip, in front of the kernels that use it.
#pragma once

template <int T>
__device__ __forceinline__ void lu_fence() { if constexpr (T > 64) __syncthreads(); else wave_fence(); }

// The family's pivot rule: largest magnitude, lowest row on ties.  Takes each thread's candidate (best, bi) of its strided column
// scan and leaves the workgroup's in every thread (s_best[4], s_bi[4]: static LDS of the kernel, used by T > 64 only).  False: the
// factorisation has broken down (a pivot that is zero, NaN or beyond 1e300); uniform over the workgroup.
template <int T>
__device__ __forceinline__ bool lu_pivot_reduce(double& best, int& bi, double* s_best, int* s_bi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  if constexpr (T > 64) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_best[wv] = best; s_bi[wv] = bi; }
    __syncthreads();
    best = s_best[0]; bi = s_bi[0];
#pragma unroll
    for (int q = 1; q < T / 64; ++q) { const double ob = s_best[q]; const int oi = s_bi[q]; if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; } }
    __syncthreads();   // s_best / s_bi are rewritten in the next step
  }
  return best > 0.0 && best < 1e300;
}

// Complex LU in place (planes Ar, Ai, row stride lda; magnitude |re| + |im|): multipliers below the diagonal.  naug further columns
// behind the matrix (an augmented right-hand side) are swapped and eliminated with their rows; perm, when not null, takes the row
// permutation, and whole rows are swapped: the multipliers already stored move with their row.
template <int T>
__device__ __forceinline__ bool clu_factor(double* Ar, double* Ai, int* perm, int nc, int lda, int naug, double* s_best, int* s_bi) {
  const int tid = threadIdx.x;
  for (int k = 0; k < nc; ++k) {
    double best = -1.0; int bi = k;
    for (int i = k + tid; i < nc; i += T) { const double v = fabs(Ar[i * lda + k]) + fabs(Ai[i * lda + k]); if (v > best) { best = v; bi = i; } }
    if (!lu_pivot_reduce<T>(best, bi, s_best, s_bi)) return false;
    if (bi != k) {
      for (int j = tid; j < nc + naug; j += T) {
        double t = Ar[k * lda + j]; Ar[k * lda + j] = Ar[bi * lda + j]; Ar[bi * lda + j] = t;
        t = Ai[k * lda + j]; Ai[k * lda + j] = Ai[bi * lda + j]; Ai[bi * lda + j] = t;
      }
      if (perm && tid == 0) { const int t = perm[k]; perm[k] = perm[bi]; perm[bi] = t; }
      lu_fence<T>();
    }
    const double pr = Ar[k * lda + k], pi = Ai[k * lda + k];
    const double den = 1.0 / (pr * pr + pi * pi), ir = pr * den, ii = -pi * den;  // 1/pivot
    for (int i = k + 1 + tid; i < nc; i += T) {
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k];
      Ar[i * lda + k] = lr * ir - li * ii; Ai[i * lda + k] = lr * ii + li * ir;
    }
    lu_fence<T>();
    const int rem = nc - k - 1, wd = rem + naug;
    for (int e = tid; e < rem * wd; e += T) {
      const int i = k + 1 + e / wd, j = k + 1 + e % wd;
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k], ur = Ar[k * lda + j], ui = Ai[k * lda + j];
      Ar[i * lda + j] -= lr * ur - li * ui; Ai[i * lda + j] -= lr * ui + li * ur;
    }
    lu_fence<T>();
  }
  return true;
}

// Forward and back substitution over the kc columns of the panel B (row stride ldb, already gathered through the permutation) on the
// factors of clu_factor: L y = P b, then U x = y
template <int T>
__device__ __forceinline__ void clu_substitute(const double* Ar, const double* Ai, double* Br, double* Bi, int nc, int lda, int kc, int ldb) {
  const int tid = threadIdx.x;
  for (int k = 0; k < nc - 1; ++k) {   // L y = P b
    const int rem = nc - k - 1;
    for (int e = tid; e < rem * kc; e += T) {
      const int i = k + 1 + e / kc, j = e % kc;
      const double lr = Ar[i * lda + k], li = Ai[i * lda + k], br = Br[k * ldb + j], bi_ = Bi[k * ldb + j];
      Br[i * ldb + j] -= lr * br - li * bi_; Bi[i * ldb + j] -= lr * bi_ + li * br;
    }
    lu_fence<T>();
  }
  for (int k = nc - 1; k >= 0; --k) {   // U x = y
    const double pr = Ar[k * lda + k], pi = Ai[k * lda + k], den = 1.0 / (pr * pr + pi * pi);
    for (int j = tid; j < kc; j += T) {
      const double br = Br[k * ldb + j], bi_ = Bi[k * ldb + j];
      Br[k * ldb + j] = (br * pr + bi_ * pi) * den; Bi[k * ldb + j] = (bi_ * pr - br * pi) * den;
    }
    lu_fence<T>();
    for (int e = tid; e < k * kc; e += T) {
      const int i = e / kc, j = e - i * kc;
      const double ur = Ar[i * lda + k], ui = Ai[i * lda + k], xr = Br[k * ldb + j], xi = Bi[k * ldb + j];
      Br[i * ldb + j] -= ur * xr - ui * xi; Bi[i * ldb + j] -= ur * xi + ui * xr;
    }
    lu_fence<T>();
  }
}

// U x = y on one column X of stride ldx (the augmented column of clu_factor with naug = 1, or a resident vector): every thread forms
// x_k in registers, thread 0 stores it
template <int T>
__device__ __forceinline__ void clu_back_column(const double* Ar, const double* Ai, double* Xr, double* Xi, int nc, int lda, int ldx) {
  const int tid = threadIdx.x;
  for (int k = nc - 1; k >= 0; --k) {
    const double pr = Ar[k * lda + k], pi = Ai[k * lda + k], br = Xr[k * ldx], bi_ = Xi[k * ldx];
    const double den = 1.0 / (pr * pr + pi * pi);
    const double xr = (br * pr + bi_ * pi) * den, xi = (bi_ * pr - br * pi) * den;
    lu_fence<T>();
    if (tid == 0) { Xr[k * ldx] = xr; Xi[k * ldx] = xi; }
    for (int i = tid; i < k; i += T) {
      const double ur = Ar[i * lda + k], ui = Ai[i * lda + k];
      Xr[i * ldx] -= ur * xr - ui * xi; Xi[i * ldx] -= ur * xi + ui * xr;
    }
    lu_fence<T>();
  }
}

// Real LU (magnitude |x|) of the augmented matrix [A | b_0 .. b_{kc-1}] (row stride lda), elimination and back substitution over all
// kc columns at once: the solutions lie in the columns nc .. nc + kc - 1.  False: broken down, the columns hold nothing.
template <int T>
__device__ __forceinline__ bool rlu_solve(double* A, int nc, int kc, int lda, double* s_best, int* s_bi) {
  const int tid = threadIdx.x;
  for (int k = 0; k < nc; ++k) {
    double best = -1.0; int bi = k;
    for (int i = k + tid; i < nc; i += T) { const double v = fabs(A[i * lda + k]); if (v > best) { best = v; bi = i; } }
    if (!lu_pivot_reduce<T>(best, bi, s_best, s_bi)) return false;
    if (bi != k) {
      for (int j = k + tid; j < nc + kc; j += T) { const double t = A[k * lda + j]; A[k * lda + j] = A[bi * lda + j]; A[bi * lda + j] = t; }
      lu_fence<T>();
    }
    const double piv = A[k * lda + k];
    for (int i = k + 1 + tid; i < nc; i += T) A[i * lda + k] /= piv;
    lu_fence<T>();
    const int rem = nc - k - 1, wd = rem + kc;
    for (int e = tid; e < rem * wd; e += T) {
      const int i = k + 1 + e / wd, j = k + 1 + e % wd;
      A[i * lda + j] -= A[i * lda + k] * A[k * lda + j];
    }
    lu_fence<T>();
  }
  for (int k = nc - 1; k >= 0; --k) {
    const double piv = A[k * lda + k];
    for (int j = tid; j < kc; j += T) A[k * lda + nc + j] /= piv;
    lu_fence<T>();
    for (int e = tid; e < k * kc; e += T) {
      const int i = e / kc, j = e - i * kc;
      A[i * lda + nc + j] -= A[i * lda + k] * A[k * lda + nc + j];
    }
    lu_fence<T>();
  }
  return true;
}
