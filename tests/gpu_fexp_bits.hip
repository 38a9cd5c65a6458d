// Stand-alone program of tests/test_gpu_fexp_bits.py: fexp of ch_bsim4.hpp against the library's exp, bit for bit, with its
// coefficients from both sources (literals, and the table in LDS that the device-resident stepper uses), in one kernel.
// Prints "points N differ_literal A differ_lds B".
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../cedarsim.jl_amd/csrc/ch_bsim4.hpp"

__global__ void fexp_bits_kernel(const double* x, long n, unsigned long long* differ) {
  __shared__ __attribute__((aligned(16))) double pool[chip::KP_COUNT];
  const chip::KLds k = chip::kpool_fill(pool, (int)threadIdx.x);
  __syncthreads();
  unsigned long long d_lit = 0, d_lds = 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const double xi = x[i], want = exp(xi), lit = chip::fexp(xi), lds = chip::fexp(xi, k);
    const bool wn = want != want;
    // NaN compared as NaN, everything else by its 64-bit pattern
    d_lit += wn ? !(lit != lit) : __double_as_longlong(lit) != __double_as_longlong(want);
    d_lds += wn ? !(lds != lds) : __double_as_longlong(lds) != __double_as_longlong(want);
  }
  if (d_lit) atomicAdd(differ, d_lit);
  if (d_lds) atomicAdd(differ + 1, d_lds);
}

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

int main() {
  std::vector<double> x;
  auto span = [&](double a, double b, long n) { for (long i = 0; i < n; ++i) x.push_back(a + (b - a) * ((double)i / (double)(n - 1))); };
  span(-40.0, 40.0, 1L << 20);
  span(-746.0, -700.0, 1L << 16);
  span(700.0, 710.0, 1L << 16);
  const double inf = std::numeric_limits<double>::infinity();
  for (double v : {0.0, -0.0, 34.0, -34.0}) { x.push_back(v); x.push_back(std::nextafter(v, inf)); x.push_back(std::nextafter(v, -inf)); }
  x.push_back(inf); x.push_back(-inf); x.push_back(std::numeric_limits<double>::quiet_NaN());
  const long n = (long)x.size();
  double* dx = nullptr; unsigned long long* dd = nullptr; unsigned long long h[2] = {0, 0};
  CHECK(hipMalloc(&dx, n * sizeof(double))); CHECK(hipMalloc(&dd, sizeof(h)));
  CHECK(hipMemcpy(dx, x.data(), n * sizeof(double), hipMemcpyHostToDevice)); CHECK(hipMemset(dd, 0, sizeof(h)));
  fexp_bits_kernel<<<256, 256>>>(dx, n, dd);
  CHECK(hipGetLastError()); CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(h, dd, sizeof(h), hipMemcpyDeviceToHost));
  std::printf("points %ld differ_literal %llu differ_lds %llu\n", n, h[0], h[1]);
  CHECK(hipFree(dx)); CHECK(hipFree(dd));
  return 0;
}
