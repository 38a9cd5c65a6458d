// Stand-alone program of tests/test_gpu_device_math.py: the DEVICE paths of csrc/va_rt.hpp (rcp / sqrt_pos / ln_pos / v_pow and
// every VD rule on top of them) and of csrc/ch_bsim4.hpp (frcp, fsqrt, flog from both constant sources, the DN<N, S> algebra in
// every combination of per-partial states) on the records of tests/device_math_cases.py, one thread per record.
//   gpu_device_math <records in> <results out>
// Both headers are found through -I, so a copy with one line changed can stand in for them.  Every operand is read from memory at
// run time and every result is stored before anything else uses it.  The host half holds the dn:: state functions, which are
// constexpr, to their definition at compile time (static_asserts below): this file does not build if one of them is wrong.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ch_bsim4.hpp"
#include "device_math_rules.hpp"

namespace dn = chip::dn;
using chip::DN;

// ---------------------------------------------------------------------------------------------------------------------------
// the state functions, over all 5 x 5 pairs.  A partial of the result may be absent only if the dense expression, evaluated with
// the zeros its operands store, is identically zero: a' + b', a' - b', a'b + ab' and (a' - q b') r are that exactly when both a'
// and b' are absent; x' c and -x' exactly when x' is.
constexpr bool absent(unsigned s) { return s < dn::PR; }
constexpr bool pair_rules_ok() {
  for (unsigned a = 0; a < 5; ++a)
    for (unsigned b = 0; b < 5; ++b) {
      const bool both = absent(a) && absent(b);
      if (absent(dn::add1(a, b)) != both || absent(dn::sub1(a, b)) != both) return false;
      if (absent(dn::mul1(a, b)) != both || absent(dn::div1(a, b)) != both) return false;
      if (absent(dn::scl1(a, b)) != absent(a)) return false;
      // the sign a sum of two literal zeros has: -0 only from (-0) + (-0) and (-0) - (+0); a zero that went through a product stays ZR
      if (both) {
        const bool zr = a == dn::ZR || b == dn::ZR;
        if (dn::add1(a, b) != (zr ? dn::ZR : ((a == dn::ZN && b == dn::ZN) ? dn::ZN : dn::ZP))) return false;
        if (dn::sub1(a, b) != (zr ? dn::ZR : ((a == dn::ZN && b == dn::ZP) ? dn::ZN : dn::ZP))) return false;
        if (dn::mul1(a, b) != dn::ZR || dn::div1(a, b) != dn::ZR) return false;
      }
      // a present result is one of the two present states
      if (!both && (dn::add1(a, b) > dn::PX || dn::sub1(a, b) > dn::PX)) return false;
    }
  for (unsigned a = 0; a < 5; ++a) {
    if (absent(dn::neg1(a)) != absent(a) || dn::neg1(dn::neg1(a)) != a) return false;
    if (a == dn::ZP && dn::neg1(a) != dn::ZN) return false;
  }
  return true;
}
static_assert(pair_rules_ok(), "dn::add1 / sub1 / mul1 / div1 / scl1 / neg1");
constexpr unsigned pack3(unsigned a, unsigned b, unsigned c) { return a | (b << 3) | (c << 6); }
constexpr bool lift_slot_mask_ok() {
  for (unsigned a = 0; a < 125; ++a) {
    const unsigned sa = pack3(a % 5, (a / 5) % 5, a / 25);
    int cnt = 0;
    for (int i = 0; i < 3; ++i) {
      if (dn::st(sa, i) != (i == 0 ? a % 5 : (i == 1 ? (a / 5) % 5 : a / 25))) return false;
      if (dn::slot(sa, i) != cnt) return false;                                  // slot = number of existing partials before i
      if ((((dn::mask(sa, 3) >> i) & 1u) != 0) != dn::has(sa, i)) return false;   // mask bit i = has(i)
      cnt += dn::has(sa, i) ? 1 : 0;
    }
    if (dn::slot(sa, 3) != cnt) return false;
    if (dn::mask(dn::from_mask(dn::mask(sa, 3), 3), 3) != dn::mask(sa, 3)) return false;
    for (int i = 0; i < 3; ++i) if (dn::st(dn::from_mask(dn::mask(sa, 3), 3), i) != (dn::has(sa, i) ? dn::PR : dn::ZR)) return false;
    for (int i = 0; i < 3; ++i) if (dn::st(dn::neg(sa, 3), i) != dn::neg1(dn::st(sa, i))) return false;
    for (unsigned b = 0; b < 25; ++b) {
      const unsigned sb = pack3(b % 5, b / 5, (a + b) % 5);
      const unsigned r = dn::lift(dn::sub1, sa, sb, 3), m = dn::lift(dn::div1, sa, sb, 3);
      for (int i = 0; i < 3; ++i) {
        if (dn::st(r, i) != dn::sub1(dn::st(sa, i), dn::st(sb, i))) return false;
        if (dn::st(m, i) != dn::div1(dn::st(sa, i), dn::st(sb, i))) return false;
      }
      if ((r >> 9) != 0) return false;
    }
  }
  return dn::all(3, dn::PR) == pack3(dn::PR, dn::PR, dn::PR) && dn::all(1, dn::ZN) == dn::ZN;
}
static_assert(lift_slot_mask_ok(), "dn::st / has / slot / mask / from_mask / lift / neg / all");
// a conversion only widens: to PR from anything, to ZR from an absent partial, otherwise to the same state
template <unsigned T> constexpr bool ok_from_row(bool z_p, bool z_n, bool z_r, bool p_r, bool p_x) {
  return DN<1, T>::ok_from(dn::ZP) == z_p && DN<1, T>::ok_from(dn::ZN) == z_n && DN<1, T>::ok_from(dn::ZR) == z_r &&
         DN<1, T>::ok_from(dn::PR) == p_r && DN<1, T>::ok_from(dn::PX) == p_x;
}
static_assert(ok_from_row<dn::PR>(true, true, true, true, true), "ok_from: to PR");
static_assert(ok_from_row<dn::ZR>(true, true, true, false, false), "ok_from: to ZR");
static_assert(ok_from_row<dn::ZP>(true, false, false, false, false), "ok_from: to ZP");
static_assert(ok_from_row<dn::ZN>(false, true, false, false, false), "ok_from: to ZN");
static_assert(ok_from_row<dn::PX>(false, false, false, false, true), "ok_from: to PX");
static_assert(DN<3, pack3(dn::PR, dn::ZR, dn::PX)>::ok_from(pack3(dn::ZN, dn::ZP, dn::PX)) &&
              !DN<3, pack3(dn::PR, dn::ZR, dn::PX)>::ok_from(pack3(dn::ZN, dn::PR, dn::PX)), "ok_from: every position counts");
static_assert(DN<3, pack3(dn::PR, dn::ZR, dn::PX)>::cnt == 2 && DN<3, pack3(dn::ZP, dn::ZN, dn::ZR)>::cnt == 0 && DN<3>::cnt == 3 &&
              DN<3, pack3(dn::PR, dn::ZR, dn::PX)>::mask == 5u, "DN::cnt / DN::mask");

// ---------------------------------------------------------------------------------------------------------------------------
// DN records: [K_DN, op, a.v, a.p0..2, b.v, b.p0..2, c, c2] -> [sparse result widened: v, p0..2 | dense result: v, p0..2],
// op = N * 10000 + form * 1000 + instantiation * 20 + operator (tests/device_math_cases.py dn_code)
// Binary instantiation J of N = 3 puts the state pairs 3J, 3J+1, 3J+2 (mod 25; pair c = (c / 5, c % 5)) on the three partials, so
// nine instantiations hold all 25; J = 9 is dense x dense.  N = 1 has one pair per instantiation.  Unary likewise over 5 states.
constexpr int NB3 = 10, NB1 = 25, NU3 = 6, NU1 = 5;
template <int N> constexpr unsigned bin_state(int j, bool right) {
  unsigned s = 0;
  for (int i = 0; i < N; ++i) {
    const int c = N == 1 ? j : (j == 9 ? 18 : (3 * j + i) % 25);
    s |= (unsigned)(right ? c % 5 : c / 5) << (3 * i);
  }
  return s;
}
template <int N> constexpr unsigned un_state(int j) {
  unsigned s = 0;
  for (int i = 0; i < N; ++i) s |= (unsigned)(N == 1 ? j : (j == 5 ? (int)dn::PR : (j + i) % 5)) << (3 * i);
  return s;
}
template <int N, unsigned S> __device__ DN<N, S> dn_load(const double* v) {
  DN<N, S> r; r.v = v[0];
  for (int i = 0; i < N; ++i) if (dn::has(S, i)) r.p[dn::slot(S, i)] = v[1 + i];
  return r;
}
template <int N, unsigned S> __device__ void dn_store(double* o, const DN<N, S>& r) {
  const DN<N> w(r);   // the widening conversion
  o[0] = w.v;
  for (int i = 0; i < 3; ++i) o[1 + i] = i < N ? w.p[i] : 0.0;
}
enum { B_ADD, B_SUB, B_MUL, B_DIV };
enum { U_NEG, U_ADD_C, U_C_ADD, U_SUB_C, U_C_SUB, U_MUL_C, U_C_MUL, U_DIV_C, U_C_DIV, U_RECIP, U_CHAIN, U_SQRT, U_EXP_LIT, U_EXP_LDS,
       U_LOG_LIT, U_LOG_LDS, U_WIDEN };

template <int N, unsigned SA, unsigned SB> __device__ void dn_binary(int op, const double* in, double* out) {
  const DN<N, SA> a = dn_load<N, SA>(in + 2);
  const DN<N, SB> b = dn_load<N, SB>(in + 6);
  const DN<N> da(a), db(b);
  switch (op) {
    case B_ADD: dn_store(out, a + b); dn_store(out + 4, da + db); break;
    case B_SUB: dn_store(out, a - b); dn_store(out + 4, da - db); break;
    case B_MUL: dn_store(out, a * b); dn_store(out + 4, da * db); break;
    case B_DIV: dn_store(out, a / b); dn_store(out + 4, da / db); break;
  }
}
template <int N, unsigned S> __device__ void dn_unary(int op, const double* in, double* out, const chip::KLds k) {
  const DN<N, S> a = dn_load<N, S>(in + 2);
  const DN<N> da(a);
  const double c = in[10], c2 = in[11];
  switch (op) {
    case U_NEG: dn_store(out, -a); dn_store(out + 4, -da); break;
    case U_ADD_C: dn_store(out, a + c); dn_store(out + 4, da + c); break;
    case U_C_ADD: dn_store(out, c + a); dn_store(out + 4, c + da); break;
    case U_SUB_C: dn_store(out, a - c); dn_store(out + 4, da - c); break;
    case U_C_SUB: dn_store(out, c - a); dn_store(out + 4, c - da); break;
    case U_MUL_C: dn_store(out, a * c); dn_store(out + 4, da * c); break;
    case U_C_MUL: dn_store(out, c * a); dn_store(out + 4, c * da); break;
    case U_DIV_C: dn_store(out, a / c); dn_store(out + 4, da / c); break;
    case U_C_DIV: dn_store(out, c / a); dn_store(out + 4, c / da); break;
    case U_RECIP: dn_store(out, chip::recip(a)); dn_store(out + 4, chip::recip(da)); break;
    case U_CHAIN: dn_store(out, chip::chain(a, c, c2)); dn_store(out + 4, chip::chain(da, c, c2)); break;
    case U_SQRT: dn_store(out, chip::dsqrt(a)); dn_store(out + 4, chip::dsqrt(da)); break;
    case U_EXP_LIT: dn_store(out, chip::dexp(a)); dn_store(out + 4, chip::dexp(da)); break;
    case U_EXP_LDS: dn_store(out, chip::dexp(a, k)); dn_store(out + 4, chip::dexp(da, k)); break;
    case U_LOG_LIT: dn_store(out, chip::dlog(a)); dn_store(out + 4, chip::dlog(da)); break;
    case U_LOG_LDS: dn_store(out, chip::dlog(a, k)); dn_store(out + 4, chip::dlog(da, k)); break;
    case U_WIDEN: dn_store(out, a); out[4] = a.v; for (int i = 0; i < 3; ++i) out[5 + i] = i < N ? a.get(i) : 0.0; break;
  }
}
template <int N, int J, int CNT> __device__ void dn_binary_at(int j, int op, const double* in, double* out) {
  if (j == J) dn_binary<N, bin_state<N>(J, false), bin_state<N>(J, true)>(op, in, out);
  else if constexpr (J + 1 < CNT) dn_binary_at<N, J + 1, CNT>(j, op, in, out);
}
template <int N, int J, int CNT> __device__ void dn_unary_at(int j, int op, const double* in, double* out, const chip::KLds k) {
  if (j == J) dn_unary<N, un_state<N>(J)>(op, in, out, k);
  else if constexpr (J + 1 < CNT) dn_unary_at<N, J + 1, CNT>(j, op, in, out, k);
}
__device__ void run_dn(const double* in, double* out, const chip::KLds k) {
  const int code = (int)in[1], n = code / 10000, form = (code / 1000) % 10, j = (code % 1000) / 20, op = code % 20;
  if (n == 3 && form == 0) dn_binary_at<3, 0, NB3>(j, op, in, out);
  else if (n == 1 && form == 0) dn_binary_at<1, 0, NB1>(j, op, in, out);
  else if (n == 3) dn_unary_at<3, 0, NU3>(j, op, in, out, k);
  else if (n == 1) dn_unary_at<1, 0, NU1>(j, op, in, out, k);
}

__device__ void run_scalar_device(const double* in, double* out, const chip::KLds k) {
  switch ((int)in[1]) {
    case dm::S_FRCP: out[0] = chip::frcp(in[2]); break;
    case dm::S_FSQRT: out[0] = chip::fsqrt(in[2]); break;
    case dm::S_FLOG: out[0] = chip::flog(in[2]); out[1] = chip::flog(in[2], k); break;
    default: break;
  }
}

__global__ void device_math_kernel(const double* in, double* out, long n) {
  __shared__ __attribute__((aligned(16))) double pool[chip::KP_COUNT];
  const chip::KLds k = chip::kpool_fill(pool, (int)threadIdx.x);
  __syncthreads();
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* r = in + i * dm::DM_NIN;
  double* o = out + i * dm::DM_NOUT;
  switch ((int)r[0]) {
    case dm::K_SCALAR: if (!dm::run_scalar_va(r, o)) run_scalar_device(r, o, k); break;
    case dm::K_VD1: dm::run_vd1(r, o); break;
    case dm::K_VD2: dm::run_vd2(r, o); break;
    case dm::K_INT: dm::run_int(r, o); break;
    case dm::K_DN: run_dn(r, o, k); break;
    case dm::K_SEED1: dm::run_seed1(r, o); break;
    default: break;
  }
}

#define CHECK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(r_)); return 2; } } while (0)

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes <= 0 || bytes % (long)(dm::DM_NIN * sizeof(double)) != 0) { std::fprintf(stderr, "bad record file (%ld bytes)\n", bytes); return 2; }
  const long n = bytes / (long)(dm::DM_NIN * sizeof(double));
  std::vector<double> in((size_t)n * dm::DM_NIN), out((size_t)n * dm::DM_NOUT);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fprintf(stderr, "short read\n"); return 2; }
  std::fclose(f);
  double *din = nullptr, *dout = nullptr;
  CHECK(hipMalloc(&din, in.size() * sizeof(double)));
  CHECK(hipMalloc(&dout, out.size() * sizeof(double)));
  CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  CHECK(hipMemset(dout, 0xff, out.size() * sizeof(double)));   // what no rule writes reads back as NaN
  const int block = 64;
  device_math_kernel<<<(unsigned)((n + block - 1) / block), block>>>(din, dout, n);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipFree(din));
  CHECK(hipFree(dout));
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::fprintf(stderr, "short write\n"); return 2; }
  if (std::fclose(f) != 0) { std::perror(argv[2]); return 2; }
  std::printf("device math gpu: %ld records\n", n);
  return 0;
}
