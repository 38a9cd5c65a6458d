// ch_engine_diag.hpp — entry-point bodies that are not part of the simulator proper: bandwidth / FP64 micro-benchmarks, the
// LDS-poisoning and device-math test hooks, single evaluations of a compiled Verilog-A module.  Included by ch_engine.hip inside
// its extern "C" block: the two kernels defined here keep their unmangled names.
#pragma once

static int ch_bench_triad_impl(ch_ctx* ctx, int64_t n, int32_t iters, double* gbps_out) {
  if (!ctx || n < 1024 || iters < 1 || !gbps_out) return CH_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  double *a = nullptr, *b = nullptr, *c = nullptr;
  const size_t bytes = (size_t)n * sizeof(double);
  if (hipMalloc((void**)&a, bytes) != hipSuccess || hipMalloc((void**)&b, bytes) != hipSuccess || hipMalloc((void**)&c, bytes) != hipSuccess) {
    (void)hipFree(a); (void)hipFree(b); (void)hipFree(c); ctx->err = "triad: out of device memory"; return CH_ERR_DEVICE;
  }
  (void)hipMemsetAsync(b, 0, bytes, ctx->stream); (void)hipMemsetAsync(c, 0, bytes, ctx->stream);
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  const int threads = 256; const long n2 = n / 2;
  const int blocks = (int)std::min<long>((n2 + threads - 1) / threads, 256L * 32);
  double best = 0;
  for (int it = 0; it <= iters; ++it) {
    (void)hipEventRecord(e0, ctx->stream);
    hipLaunchKernelGGL(triad_kernel, dim3(blocks), dim3(threads), 0, ctx->stream, (double2*)a, (const double2*)b, (const double2*)c, 3.0, n2);
    (void)hipEventRecord(e1, ctx->stream);
    if (hipEventSynchronize(e1) != hipSuccess) { ctx->err = "triad kernel failed"; break; }
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    if (it > 0 && ms > 0) best = std::max(best, 3.0 * (double)(n2 * 2) * sizeof(double) / (ms * 1e-3) / 1e9);
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(a); (void)hipFree(b); (void)hipFree(c);
  *gbps_out = best;
  return best > 0 ? CH_OK : CH_ERR_DEVICE;
}
// Test hook: fills the LDS of every CU with a pattern that is a NaN as a double and a large negative number as an int, so that a
// kernel which reads LDS it has not staged itself (LDS keeps whatever the previous kernel left there) gets garbage deterministically
// instead of the zeros of a fresh process.  The round-2 abort of test_gpu_stepper.py (gpurun_out/r02_stepper6.log) was exactly
// that: the helper wave of a pair read its OWN, unstaged slot table after a host-stepper kernel had used the CU.
__global__ void poison_lds_kernel(unsigned* sink) {
  extern __shared__ unsigned pl_[];
  const int n = LDS_BYTES_PER_CU / 4 - 64;
  for (int i = threadIdx.x; i < n; i += blockDim.x) pl_[i] = 0xfff7a5a5u;
  __syncthreads();
  if (threadIdx.x == 0 && pl_[blockIdx.x % n] != 0xfff7a5a5u) *sink = 1u;   // keeps the stores alive
}
static int ch_debug_poison_lds_impl(ch_ctx* ctx) {
  if (!ctx) return CH_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return CH_ERR_DEVICE;
  unsigned* sink = nullptr;
  if (hipMalloc((void**)&sink, sizeof(unsigned)) != hipSuccess) return CH_ERR_DEVICE;
  const int lds = LDS_BYTES_PER_CU - 256;
  (void)hipFuncSetAttribute((const void*)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  // one workgroup fills a CU's LDS; several rounds of n_cu workgroups so that every CU is reached whatever the dispatcher does
  hipLaunchKernelGGL(poison_lds_kernel, dim3(prop.multiProcessorCount * 8), dim3(256), lds, ctx->stream, sink);
  const hipError_t e = hipStreamSynchronize(ctx->stream);
  (void)hipFree(sink);
  if (e != hipSuccess) { ctx->err = std::string("poison_lds: ") + hipGetErrorString(e); return CH_ERR_DEVICE; }
  return CH_OK;
}
// test hook: the device's own exp / ln (va::v_exp, va::v_ln of va_rt.hpp and the BSIM4 code's flog) over a vector
__global__ void debug_math_kernel(int which, int n, const double* x, double* y) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = which == 0 ? va::v_exp(x[i]) : which == 1 ? va::v_ln(x[i]) : flog(x[i]);
}
static int ch_debug_math_impl(ch_ctx* ctx, int32_t which, int32_t n, const double* x, double* y) {
  if (!ctx || which < 0 || which > 2 || n < 1 || !x || !y) return CH_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  double *dx = nullptr, *dy = nullptr;
  if (hipMalloc((void**)&dx, (size_t)n * sizeof(double)) != hipSuccess || hipMalloc((void**)&dy, (size_t)n * sizeof(double)) != hipSuccess) { (void)hipFree(dx); return CH_ERR_NOMEM; }
  hipError_t e = hipMemcpy(dx, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) { hipLaunchKernelGGL(debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, which, n, (const double*)dx, dy); e = hipStreamSynchronize(ctx->stream); }
  if (e == hipSuccess) e = hipMemcpy(y, dy, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dy);
  if (e != hipSuccess) { ctx->err = std::string("debug_math: ") + hipGetErrorString(e); return CH_ERR_DEVICE; }
  return CH_OK;
}
static int ch_bench_fp64_impl(ch_ctx* ctx, int32_t iters, double* tflops_out) {
  if (!ctx || iters < 1 || !tflops_out) return CH_ERR_INVALID;
  (void)hipSetDevice(ctx->device);
  hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return CH_ERR_DEVICE;
  const int blocks = prop.multiProcessorCount * 8, threads = 256, n_outer = 2000;  // 8 waves per SIMD
  double* out = nullptr;
  if (hipMalloc((void**)&out, (size_t)blocks * threads * sizeof(double)) != hipSuccess) return CH_ERR_DEVICE;
  hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  double best = 0;
  for (int it = 0; it <= iters; ++it) {
    (void)hipEventRecord(e0, ctx->stream);
    hipLaunchKernelGGL(fp64_peak_kernel, dim3(blocks), dim3(threads), 0, ctx->stream, out, n_outer, 0.999999, 1e-6);
    (void)hipEventRecord(e1, ctx->stream);
    if (hipEventSynchronize(e1) != hipSuccess) { ctx->err = "fp64 peak kernel failed"; break; }
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    const double flop = 2.0 * 16 * 8 * (double)n_outer * blocks * threads;
    if (it > 0 && ms > 0) best = std::max(best, flop / (ms * 1e-3) / 1e12);
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); (void)hipFree(out);
  *tflops_out = best;
  return best > 0 ? CH_OK : CH_ERR_DEVICE;
}
// one compiled module on one wavefront (va_eval_kernel / va_opvars_kernel): parameters and terminal voltages up, `n_out` doubles back
static int va_run_one(ch_ctx* ctx, void (*kernel)(int, const double*, const double*, double, double, double*), int32_t id, const double* par, const double* v,
                      double temperature_k, double gmin, double* out, size_t n_out) {
  (void)hipSetDevice(ctx->device);
  const va_gen::ModuleInfo& mi = va_gen::MODULES[id];
  double *dp = nullptr, *dv = nullptr, *dout = nullptr;
  if (hipMalloc((void**)&dp, (size_t)std::max(1, 2 * mi.n_params) * sizeof(double)) != hipSuccess || hipMalloc((void**)&dv, NTERM * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&dout, n_out * sizeof(double)) != hipSuccess) return CH_ERR_DEVICE;
  double vv[NTERM] = {0}; for (int k = 0; k < mi.n_nodes; ++k) vv[k] = v[k];
  (void)hipMemcpy(dp, par, (size_t)2 * mi.n_params * sizeof(double), hipMemcpyHostToDevice);
  (void)hipMemcpy(dv, vv, sizeof(vv), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, ctx->stream, (int)id, (const double*)dp, (const double*)dv, temperature_k, gmin, dout);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, dout, n_out * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dp); (void)hipFree(dv); (void)hipFree(dout);
  if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return CH_ERR_DEVICE; }
  return CH_OK;
}
static int ch_va_eval_impl(ch_ctx* ctx, int32_t id, const double* par, const double* v, double temperature_k, double gmin, double* st_out) {
  if (!ctx || !par || !v || !st_out || id < 0 || id >= va_gen::N_MODULES) return CH_ERR_INVALID;
  return va_run_one(ctx, va_eval_kernel, id, par, v, temperature_k, gmin, st_out, 144);
}
static int ch_va_opvars_impl(ch_ctx* ctx, int32_t id, const double* par, const double* v, double temperature_k, double gmin, double* op_out) {
  if (!ctx || !par || !v || !op_out || id < 0 || id >= va_gen::N_MODULES) return CH_ERR_INVALID;
  const int nop = va_gen::N_OPVARS[id];
  return nop == 0 ? CH_OK : va_run_one(ctx, va_opvars_kernel, id, par, v, temperature_k, gmin, op_out, (size_t)nop);
}
