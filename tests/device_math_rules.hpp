// The rules of csrc/va_rt.hpp as tests/device_math_cases.py numbers them, shared by tests/host_device_math.cpp (library path, g++)
// and tests/gpu_device_math.hip (device path, gfx950).  One record in: [kind, rule, x, y, c, aux, ...] (DM_NIN doubles); one record
// out: DM_NOUT doubles.  Every operand is read from the record and every result is written to it: nothing is folded at compile
// time and no contraction crosses two rules.
#pragma once
#include "va_rt.hpp"

namespace dm {

constexpr int DM_NIN = 12, DM_NOUT = 16;
enum Kind { K_SCALAR = 0, K_VD1 = 1, K_VD2 = 2, K_INT = 3, K_DN = 4, K_SEED1 = 5 };

// kind K_VD1 / K_VD2: T f(T x, T y, double c); x is variable 0, y is variable 1
enum Rule {
  R_EXP, R_LN, R_LOG10, R_SQRT, R_SIN, R_COS, R_TAN, R_SINH, R_COSH, R_TANH, R_ATAN, R_ASIN, R_ACOS, R_ASINH, R_ACOSH, R_ATANH,
  R_ABS, R_FLOOR, R_CEIL, R_LIMEXP, R_RCP, R_NEG,
  R_ADD, R_SUB, R_MUL, R_DIV, R_VDIV, R_MIN, R_MAX, R_HYPOT, R_ATAN2, R_POW_VV, R_ADD_ASSIGN, R_SUB_ASSIGN,
  R_ADD_VC, R_ADD_CV, R_ADD_VI, R_ADD_IV, R_SUB_VC, R_SUB_CV, R_SUB_VI, R_SUB_IV,
  R_MUL_VC, R_MUL_CV, R_MUL_VI, R_MUL_IV, R_DIV_VC, R_DIV_CV, R_DIV_VI, R_DIV_IV,
  R_VDIV_VC, R_VDIV_CV, R_POW_VC, R_POW_VI, R_POW_CV, R_SEED, R_COUNT
};
// kind K_SCALAR
enum Scalar { S_RCP, S_FRCP, S_VDIV, S_SQRT, S_FSQRT, S_FLOG, S_POW, S_LIMEXP, S_HYPOT, S_ATAN2, S_MIN, S_MAX, S_ABS, S_LN, S_LOG10,
              S_ASIN, S_ACOS, S_ACOSH, S_ATANH };
// kind K_INT
enum Int { I_TO_INT, I_CLAMP, I_TRUTH, I_ABS_INT, I_MINMAX_INT };

template <class T>
VA_HD_NOINLINE T apply(int rule, const T& x, const T& y, double c) {
  const int ci = (int)c;
  switch (rule) {
    case R_EXP: return va::v_exp(x);
    case R_LN: return va::v_ln(x);
    case R_LOG10: return va::v_log10(x);
    case R_SQRT: return va::v_sqrt(x);
    case R_SIN: return va::v_sin(x);
    case R_COS: return va::v_cos(x);
    case R_TAN: return va::v_tan(x);
    case R_SINH: return va::v_sinh(x);
    case R_COSH: return va::v_cosh(x);
    case R_TANH: return va::v_tanh(x);
    case R_ATAN: return va::v_atan(x);
    case R_ASIN: return va::v_asin(x);
    case R_ACOS: return va::v_acos(x);
    case R_ASINH: return va::v_asinh(x);
    case R_ACOSH: return va::v_acosh(x);
    case R_ATANH: return va::v_atanh(x);
    case R_ABS: return va::v_abs(x);
    case R_FLOOR: return T(va::v_floor(x));
    case R_CEIL: return T(va::v_ceil(x));
    case R_LIMEXP: return va::v_limexp(x);
    case R_RCP: return va::rcp(x);
    case R_NEG: return -x;
    case R_ADD: return x + y;
    case R_SUB: return x - y;
    case R_MUL: return x * y;
    case R_DIV: return x / y;
    case R_VDIV: return va::v_div(x, y);
    case R_MIN: return va::v_min(x, y);
    case R_MAX: return va::v_max(x, y);
    case R_HYPOT: return va::v_hypot(x, y);
    case R_ATAN2: return va::v_atan2(x, y);   // atan2(first, second)
    case R_POW_VV: return va::v_pow(x, y);
    case R_ADD_ASSIGN: { T r = x; r += y; return r; }
    case R_SUB_ASSIGN: { T r = x; r -= y; return r; }
    case R_ADD_VC: return x + c;
    case R_ADD_CV: return c + x;
    case R_ADD_VI: return x + ci;
    case R_ADD_IV: return ci + x;
    case R_SUB_VC: return x - c;
    case R_SUB_CV: return c - x;
    case R_SUB_VI: return x - ci;
    case R_SUB_IV: return ci - x;
    case R_MUL_VC: return x * c;
    case R_MUL_CV: return c * x;
    case R_MUL_VI: return x * ci;
    case R_MUL_IV: return ci * x;
    case R_DIV_VC: return x / c;
    case R_DIV_CV: return c / x;
    case R_DIV_VI: return x / ci;
    case R_DIV_IV: return ci / x;
    case R_VDIV_VC: return va::v_div(x, c);
    case R_VDIV_CV: return va::v_div(c, x);
    case R_POW_VC: return va::v_pow(x, c);
    case R_POW_VI: return va::v_pow(x, ci);
    case R_POW_CV: return va::v_pow(c, x);
    case R_SEED: return x;
    default: return T(NAN);
  }
}

typedef va::VD<2, double> T1;
typedef va::VD<2, T1> T2;

VA_HD_NOINLINE void run_vd1(const double* in, double* out) {
  const T1 x = va::seed(in[2], 0, -1, (T1*)nullptr), y = va::seed(in[3], 1, -1, (T1*)nullptr);
  const T1 r = apply<T1>((int)in[1], x, y, in[4]);
  out[0] = r.v; out[1] = r.d[0]; out[2] = r.d[1];
}

VA_HD_NOINLINE void run_vd2(const double* in, double* out) {
  const T2 x = va::seed(in[2], 0, 0, (T2*)nullptr), y = va::seed(in[3], 1, 1, (T2*)nullptr);
  const T2 r = apply<T2>((int)in[1], x, y, in[4]);
  out[0] = r.v.v; out[1] = r.v.d[0]; out[2] = r.v.d[1];
  out[3] = r.d[0].v; out[4] = r.d[1].v;
  out[5] = r.d[0].d[0]; out[6] = r.d[0].d[1]; out[7] = r.d[1].d[0]; out[8] = r.d[1].d[1];
  const T2 p = va::ddx1(r, 0), q = va::ddx2(r, 0, 1);
  out[9] = p.v.v; out[10] = p.d[0].v; out[11] = p.d[1].v;
  out[12] = q.v.v; out[13] = q.d[0].v; out[14] = q.d[1].v;
  out[15] = va::ddx1(in[2], 0) + va::ddx2(in[2], 0, 1) + p.v.d[0] + p.v.d[1] + q.d[0].d[0] + q.d[1].d[1];   // all zero by definition
}

// sin of a one-directional seed: x = in[2], is_dir = in[3] != 0, dk = (int)in[4] (-1: no inner variable)
VA_HD_NOINLINE void run_seed1(const double* in, double* out) {
  typedef va::VD<1, double> U1;
  typedef va::VD<1, T1> U2;
  const U1 a = va::v_sin(va::seed1(in[2], in[3] != 0.0, (int)in[4], (U1*)nullptr));
  const U2 b = va::v_sin(va::seed1(in[2], in[3] != 0.0, (int)in[4], (U2*)nullptr));
  out[0] = a.v; out[1] = a.d[0];
  out[2] = b.v.v; out[3] = b.v.d[0]; out[4] = b.v.d[1]; out[5] = b.d[0].v; out[6] = b.d[0].d[0]; out[7] = b.d[0].d[1];
}

VA_HD_NOINLINE void run_int(const double* in, double* out) {
  const double x = in[2];
  switch ((int)in[1]) {
    case I_TO_INT:
      out[0] = (double)va::to_int(x); out[1] = (double)va::to_int(T1(x)); out[2] = (double)va::to_int(T2(x)); out[3] = (double)va::to_int((int)in[3]);
      break;
    case I_CLAMP: out[0] = (double)va::clamp_index((int)in[2], (int)in[3], (int)in[4]); break;
    case I_TRUTH:
      out[0] = va::truth(x) ? 1.0 : 0.0; out[1] = va::truth((int)in[3]) ? 1.0 : 0.0; out[2] = va::truth(in[4] != 0.0) ? 1.0 : 0.0;
      out[3] = va::truth(T1(x)) ? 1.0 : 0.0; out[4] = va::truth(T2(x)) ? 1.0 : 0.0;
      break;
    case I_ABS_INT: out[0] = (double)va::v_abs((int)in[2]); break;
    case I_MINMAX_INT: out[0] = (double)va::v_min((int)in[2], (int)in[3]); out[1] = (double)va::v_max((int)in[2], (int)in[3]); break;
  }
}

// the scalars that exist on both sides; returns false for a rule only the device has
VA_HD_NOINLINE bool run_scalar_va(const double* in, double* out) {
  const double a = in[2], b = in[3];
  switch ((int)in[1]) {
    case S_RCP: out[0] = va::rcp(a); return true;
    case S_VDIV: out[0] = va::v_div(a, b); return true;
    case S_SQRT: out[0] = va::v_sqrt(a); return true;
    case S_POW: out[0] = va::v_pow(a, b); return true;
    case S_LIMEXP: out[0] = va::v_limexp(a); return true;
    case S_HYPOT: out[0] = va::v_hypot(a, b); return true;
    case S_ATAN2: out[0] = va::v_atan2(a, b); return true;
    case S_MIN: out[0] = va::v_min(a, b); return true;
    case S_MAX: out[0] = va::v_max(a, b); return true;
    case S_ABS: out[0] = va::v_abs(a); return true;
    case S_LN: out[0] = va::v_ln(a); return true;
    case S_LOG10: out[0] = va::v_log10(a); return true;
    case S_ASIN: out[0] = va::v_asin(a); return true;
    case S_ACOS: out[0] = va::v_acos(a); return true;
    case S_ACOSH: out[0] = va::v_acosh(a); return true;
    case S_ATANH: out[0] = va::v_atanh(a); return true;
    default: return false;
  }
}

}  // namespace dm
