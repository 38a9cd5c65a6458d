// ch_bsim4.hpp — BSIM4 (level 54, v4.5) MOSFET for the HIP engine.
//
// Replaces the VA-generated device functor the reference evaluates per instance per residual call
// (src/vasim.jl:853-867; `bsim4.va` from package BSIM4 0.5.0, used at test/gf180_dff.jl:11,
// benchmarks/benchmark_common.jl:57).  Two halves:
//   * b4_pack()   host: card ⊕ instance ⊕ temperature → packed parameter column (what the
//                 reference constant-folds per instance), one column per distinct
//                 (model, W, L, NF, AS, AD, PS, PD[, sample]) class;
//   * b4_device() device: one lane evaluates one instance.  The core is differentiated with a
//                 3-partial dual number in the MODE frame (Vgs', Vds', Vbs' after source/drain
//                 interchange) and chained to the 4x4 terminal stamp once at the end; junction
//                 diodes, junction charges and overlap charges are 1-D functions with analytic
//                 derivatives.  (The reference uses ForwardDiff duals on all of it,
//                 src/vasim.jl:347-357.)
// The model equations are the public BSIM4.5.0 definition for mobMod 0/1/2, capMod 2 (and 0 = no
// intrinsic charge), dioMod 1, rdsMod 0, no gate current / NQS / rgate / rbody.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/cedarhip.h"
#include "ch_b4_noise.hpp"

#if defined(__HIPCC__)
#define CH_HD __host__ __device__
#define CH_D __device__ __forceinline__
#else
#define CH_HD
#define CH_D inline
#endif

namespace chip {

// Packed per-class parameter column.  X(name)
#define CH_B4_PACKED(X)                                                                              \
  X(type) X(mobmod) X(capmod) X(nf) X(leff) X(weff) X(weffCV) X(weffCJ) X(vtm) X(tratio1) X(toxe)    \
  X(coxe) X(coxp) X(factor1) X(phi) X(sqrtPhi) X(Xdep0) X(vbi_phi) X(cdep0) X(litl) X(ldeb) X(k1)    \
  X(k1ox) X(k2ox) X(vbsc) X(vfb_phi) X(vth0t) X(k3) X(k3b) X(vthNarrowW) X(lpe0term) X(LpeVb)        \
  X(dvt0) X(dvt1L) X(dvt2) X(dvt0w) X(dvt1wWL) X(dvt2w) X(eta0) X(etab) X(kt1eff) X(kt2t)            \
  X(theta0vb0) X(thetaRout) X(vfbzb) X(vtfbphi1) X(vtfbphi2) X(nfactor) X(cdsc) X(cdscb) X(cdscd)    \
  X(cit) X(voffcbn) X(mstar) X(ngate) X(polyT1) X(dvtp0) X(dvtp1) X(ua) X(ub) X(uc) X(u0temp) X(eu)  \
  X(vsattemp) X(a0) X(agsa0) X(a1) X(a2) X(b0term) X(keta) X(xj) X(dwg) X(dwb) X(rds0h) X(rdswmin)   \
  X(prwg) X(prwb) X(delta) X(pclmlitl) X(pdiblb) X(fproutL) X(pdits) X(pditsd) X(pditslL) X(pscbe1l) \
  X(pscbe2) X(pvag) X(alphaL) X(beta0) X(agidlW) X(bgidl) X(cgidl) X(egidl) X(toxe3) X(xpart)        \
  X(cgso) X(cgdo) X(cgbo) X(cgslW) X(cgdlW) X(ckappas) X(ckappad) X(abulkCVfactor) X(acde) X(moinVtm) \
  X(noff) X(voffcv) X(CoxWL) X(toxp8) X(Isbs) X(Isbd) X(Nvtms) X(Nvtmd) X(vjsmFwd) X(vjdmFwd)        \
  X(IVjsmFwd) X(IVjdmFwd) X(czbs) X(czbssw) X(czbsswg) X(czbd) X(czbdsw) X(czbdswg) X(PhiBS)         \
  X(PhiBSWS) X(PhiBSWGS) X(PhiBD) X(PhiBSWD) X(PhiBSWGD) X(mjs) X(mjsws) X(mjswgs) X(mjd) X(mjswd)   \
  X(mjswgd)

enum B4Idx {
#define X(n) B4I_##n,
  CH_B4_PACKED(X)
#undef X
      B4I_COUNT
};

namespace k {
constexpr double EPS0 = 8.85418e-12, EPSSI = 1.03594e-10, KboQ = 8.617087e-5, Q = 1.60219e-19;
constexpr double MAX_EXP = 5.834617425e14, MIN_EXP = 1.713908431e-15, EXP_TH = 34.0;
constexpr double PI = 3.14159265358979323846;
}  // namespace k

// ------------------------------------------------------------------------------------------------
// Host: build one packed column.  mp = model card (CH_B4_NPAR, NaN = not given),
// ip = instance {w,l,nf,as,ad,ps,pd} (already multiplied by .option scale), temp in Celsius.
inline int b4_pack(const double* mp, const double* ip, double temp_c, double* out) {
  using namespace k;
  auto has = [&](int i) { return !std::isnan(mp[i]); };
  auto par = [&](int i, double d) { return std::isnan(mp[i]) ? d : mp[i]; };
  for (int i = 0; i < B4I_COUNT; ++i) out[i] = 0.0;
#define O(n) out[B4I_##n]
  const double type = par(CH_B4_type, 1.0);
  const int mobmod = (int)par(CH_B4_mobmod, 0.0), capmod = (int)par(CH_B4_capmod, 2.0);
  const int permod = (int)par(CH_B4_permod, 1.0), binunit = (int)par(CH_B4_binunit, 1.0);
  if ((int)par(CH_B4_rdsmod, 0.0) != 0 || (int)par(CH_B4_rgatemod, 0.0) != 0 || (int)par(CH_B4_rbodymod, 0.0) != 0 ||
      (int)par(CH_B4_igcmod, 0.0) != 0 || (int)par(CH_B4_igbmod, 0.0) != 0 || (int)par(CH_B4_trnqsmod, 0.0) != 0 ||
      (int)par(CH_B4_geomod, 0.0) != 0 || (int)par(CH_B4_diomod, 1.0) != 1 || mobmod < 0 || mobmod > 2 ||
      !(capmod == 0 || capmod == 2))
    return CH_ERR_UNSUPPORTED;
  const double W = ip[CH_MOS_W], L = ip[CH_MOS_L];
  const double nf = std::isnan(ip[CH_MOS_NF]) ? 1.0 : ip[CH_MOS_NF];
  if (!(W > 0) || !(L > 0) || !(nf >= 1)) return CH_ERR_INVALID;

  // temperatures
  const double Tn = par(CH_B4_tnom, 27.0) + 273.15, T = temp_c + 273.15;
  const double tr = T / Tn, dT = T - Tn, vtm0 = KboQ * Tn, vtm = KboQ * T;
  const double Eg0 = 1.16 - 7.02e-4 * Tn * Tn / (Tn + 1108.0), Eg = 1.16 - 7.02e-4 * T * T / (T + 1108.0);
  const double ni = 1.45e10 * (Tn / 300.15) * std::sqrt(Tn / 300.15) * std::exp(21.5565981 - Eg0 / (2.0 * vtm0));
  // oxide
  const double toxe = par(CH_B4_toxe, 3e-9), toxp = par(CH_B4_toxp, toxe), toxm = par(CH_B4_toxm, toxe);
  const double epsrox = par(CH_B4_epsrox, 3.9), coxe = epsrox * EPS0 / toxe, coxp = epsrox * EPS0 / toxp;
  const double factor1 = std::sqrt(EPSSI / (epsrox * EPS0) * toxe);
  // effective dimensions
  const double lint = par(CH_B4_lint, 0), wint = par(CH_B4_wint, 0);
  const double ll = par(CH_B4_ll, 0), lw = par(CH_B4_lw, 0), lwl = par(CH_B4_lwl, 0);
  const double wl = par(CH_B4_wl, 0), ww = par(CH_B4_ww, 0), wwl = par(CH_B4_wwl, 0);
  const double lln = par(CH_B4_lln, 1), lwn = par(CH_B4_lwn, 1), wln = par(CH_B4_wln, 1), wwn = par(CH_B4_wwn, 1);
  const double dlc0 = par(CH_B4_dlc, lint), dwc0 = par(CH_B4_dwc, wint), dwj0 = par(CH_B4_dwj, dwc0);
  const double Ln = L + par(CH_B4_xl, 0), Wn = W / nf + par(CH_B4_xw, 0);
  const double pl1 = std::pow(Ln, lln), pw1 = std::pow(Wn, lwn), pl2 = std::pow(Ln, wln), pw2 = std::pow(Wn, wwn);
  const double dl = lint + ll / pl1 + lw / pw1 + lwl / (pl1 * pw1);
  const double dlc = dlc0 + par(CH_B4_llc, ll) / pl1 + par(CH_B4_lwc, lw) / pw1 + par(CH_B4_lwlc, lwl) / (pl1 * pw1);
  const double dw = wint + wl / pl2 + ww / pw2 + wwl / (pl2 * pw2);
  const double dwx = par(CH_B4_wlc, wl) / pl2 + par(CH_B4_wwc, ww) / pw2 + par(CH_B4_wwlc, wwl) / (pl2 * pw2);
  const double leff = Ln - 2 * dl, weff = Wn - 2 * dw, leffCV = Ln - 2 * dlc, weffCV = Wn - 2 * (dwc0 + dwx),
               weffCJ = Wn - 2 * (dwj0 + dwx);
  if (leff <= 0 || weff <= 0 || leffCV <= 0 || weffCV <= 0 || weffCJ <= 0) return CH_ERR_INVALID;
  const double iL = (binunit == 1 ? 1e-6 : 1.0) / leff, iW = (binunit == 1 ? 1e-6 : 1.0) / weff, iLW = iL * iW;
  auto bin = [&](int i, double d) {
    auto z = [&](int j) { return std::isnan(mp[j]) ? 0.0 : mp[j]; };
    return par(i, d) + z(i + 1) * iL + z(i + 2) * iW + z(i + 3) * iLW;
  };
  // binned card values
  const double xj = bin(CH_B4_xj, 1.5e-7), ndep = bin(CH_B4_ndep, 1.7e17), nsd = bin(CH_B4_nsd, 1e20);
  const double nsub = bin(CH_B4_nsub, 6e16), ngate = bin(CH_B4_ngate, 0), phin = bin(CH_B4_phin, 0);
  double vbm = bin(CH_B4_vbm, -3.0);
  const double lpe0 = bin(CH_B4_lpe0, 1.74e-7), lpeb = bin(CH_B4_lpeb, 0), w0 = bin(CH_B4_w0, 2.5e-6);
  const double k3 = bin(CH_B4_k3, 80.0), k3b = bin(CH_B4_k3b, 0);
  const double dvt0 = bin(CH_B4_dvt0, 2.2), dvt1 = bin(CH_B4_dvt1, 0.53), dvt2 = bin(CH_B4_dvt2, -0.032);
  const double dvt0w = bin(CH_B4_dvt0w, 0), dvt1w = bin(CH_B4_dvt1w, 5.3e6), dvt2w = bin(CH_B4_dvt2w, -0.032);
  const double drout = bin(CH_B4_drout, 0.56), dsub = has(CH_B4_dsub) ? bin(CH_B4_dsub, 0) : drout;
  const double kt1 = bin(CH_B4_kt1, -0.11), kt1l = bin(CH_B4_kt1l, 0), kt2 = bin(CH_B4_kt2, 0.022);
  double u0 = bin(CH_B4_u0, type > 0 ? 0.067 : 0.025);
  if (u0 > 1.0) u0 *= 1e-4;
  const double tr1 = tr - 1.0;
  O(type) = type; O(mobmod) = mobmod; O(capmod) = capmod; O(nf) = nf;
  O(leff) = leff; O(weff) = weff; O(weffCV) = weffCV; O(weffCJ) = weffCJ;
  O(vtm) = vtm; O(tratio1) = tr1; O(toxe) = toxe; O(coxe) = coxe; O(coxp) = coxp; O(factor1) = factor1;
  const double phi = vtm0 * std::log(ndep / ni) + phin + 0.4, sqrtPhi = std::sqrt(phi);
  O(phi) = phi; O(sqrtPhi) = sqrtPhi;
  const double Xdep0 = std::sqrt(2.0 * EPSSI / (Q * ndep * 1e6)) * sqrtPhi;
  O(Xdep0) = Xdep0;
  const double vbi = vtm0 * std::log(nsd * ndep / (ni * ni));
  O(vbi_phi) = vbi - phi;
  O(cdep0) = std::sqrt(Q * EPSSI * ndep * 1e6 / 2.0 / phi);
  const double litl = std::sqrt(3.0 * xj * toxe);
  O(litl) = litl;
  O(ldeb) = std::sqrt(EPSSI * vtm0 / (Q * ndep * 1e6)) / 3.0;
  double k1, k2;
  if (has(CH_B4_k1) || has(CH_B4_k2)) { k1 = bin(CH_B4_k1, 0.53); k2 = bin(CH_B4_k2, -0.0186); }
  else {
    const double g1 = has(CH_B4_gamma1) ? bin(CH_B4_gamma1, 0) : 5.753e-12 * std::sqrt(ndep) / coxe;
    const double g2 = has(CH_B4_gamma2) ? bin(CH_B4_gamma2, 0) : 5.753e-12 * std::sqrt(nsub) / coxe;
    const double xt = bin(CH_B4_xt, 1.55e-7);
    double vbx = has(CH_B4_vbx) ? bin(CH_B4_vbx, 0) : phi - 7.7348e-4 * ndep * xt * xt;
    if (vbx > 0) vbx = -vbx;
    if (vbm > 0) vbm = -vbm;
    const double a = std::sqrt(phi - vbx) - sqrtPhi, b = std::sqrt(phi * (phi - vbm)) - phi;
    k2 = (g1 - g2) * a / (2.0 * b + vbm);
    k1 = g2 - 2.0 * k2 * std::sqrt(phi - vbm);
  }
  double vbsc = -30.0;
  if (k2 < 0) { const double h = 0.5 * k1 / k2; vbsc = 0.9 * (phi - h * h); vbsc = vbsc > -3.0 ? -3.0 : (vbsc < -30.0 ? -30.0 : vbsc); }
  if (vbsc > vbm) vbsc = vbm;
  const double k1ox = k1 * toxe / toxm, k2ox = k2 * toxe / toxm;
  O(k1) = k1; O(k1ox) = k1ox; O(k2ox) = k2ox; O(vbsc) = vbsc;
  const bool vth0Given = has(CH_B4_vth0);
  double vth0 = bin(CH_B4_vth0, type > 0 ? 0.7 : -0.7), vfb;
  if (has(CH_B4_vfb)) vfb = bin(CH_B4_vfb, -1.0);
  else if (vth0Given) vfb = type * vth0 - phi - k1 * sqrtPhi;
  else vfb = -1.0;
  if (!vth0Given) vth0 = type * (vfb + phi + k1ox * sqrtPhi);
  O(vfb_phi) = vfb + phi;
  O(vth0t) = type * vth0;
  O(k3) = k3; O(k3b) = k3b;
  const double vthNW = toxe * phi / (weff + w0);
  O(vthNarrowW) = vthNW;
  const double lpe0s = std::sqrt(1.0 + lpe0 / leff);
  O(lpe0term) = k1ox * (lpe0s - 1.0) * sqrtPhi;
  O(LpeVb) = std::sqrt(1.0 + lpeb / leff);
  O(dvt0) = dvt0; O(dvt1L) = dvt1 * leff; O(dvt2) = dvt2;
  O(dvt0w) = dvt0w; O(dvt1wWL) = dvt1w * weff * leff; O(dvt2w) = dvt2w;
  O(eta0) = bin(CH_B4_eta0, 0.08); O(etab) = bin(CH_B4_etab, -0.07);
  O(kt1eff) = (kt1 + kt1l / leff) * tr1; O(kt2t) = kt2 * tr1;
  auto sce = [&](double x) {
    if (x < EXP_TH) { const double e = std::exp(x), m1 = e - 1.0; return e / (m1 * m1 + 2.0 * e * MIN_EXP); }
    return 1.0 / (MAX_EXP - 2.0);
  };
  const double lt0 = std::sqrt(EPSSI / (epsrox * EPS0) * toxe * Xdep0);
  O(theta0vb0) = sce(dsub * leff / lt0);
  O(thetaRout) = bin(CH_B4_pdiblc1, 0.39) * sce(drout * leff / lt0) + bin(CH_B4_pdiblc2, 0.0086);
  {
    const double v0 = vbi - phi, f1x = factor1 * std::sqrt(Xdep0);
    const double t8 = dvt0w * sce(dvt1w * weff * leff / f1x) * v0, t9 = dvt0 * sce(dvt1 * leff / f1x) * v0;
    const double t5 = k1ox * (lpe0s - 1.0) * sqrtPhi + (kt1 + kt1l / leff) * tr1;
    O(vfbzb) = type * vth0 - t8 - t9 + k3 * vthNW + t5 - phi - k1 * sqrtPhi;
  }
  {
    const double t3 = type * vth0 - vfb - phi;
    double a = type > 0 ? 2.0 * t3 : 2.5 * t3, b = 4.0 * t3;
    O(vtfbphi1) = a < 0 ? 0 : a; O(vtfbphi2) = b < 0 ? 0 : b;
  }
  O(nfactor) = bin(CH_B4_nfactor, 1.0); O(cdsc) = bin(CH_B4_cdsc, 2.4e-4); O(cdscb) = bin(CH_B4_cdscb, 0);
  O(cdscd) = bin(CH_B4_cdscd, 0); O(cit) = bin(CH_B4_cit, 0);
  O(voffcbn) = (bin(CH_B4_voff, -0.08) + par(CH_B4_voffl, 0) / leff) * (1.0 + bin(CH_B4_tvoff, 0) * dT);
  O(mstar) = 0.5 + std::atan(bin(CH_B4_minv, 0)) / PI;
  O(ngate) = ngate;
  O(polyT1) = 1e6 * Q * EPSSI * ngate / (coxe * coxe);
  O(dvtp0) = bin(CH_B4_dvtp0, 0); O(dvtp1) = bin(CH_B4_dvtp1, 0);
  O(ua) = bin(CH_B4_ua, mobmod == 2 ? 1e-15 : 1e-9) + bin(CH_B4_ua1, 1e-9) * tr1;
  O(ub) = bin(CH_B4_ub, 1e-19) + bin(CH_B4_ub1, -1e-18) * tr1;
  O(uc) = bin(CH_B4_uc, mobmod == 1 ? -0.0465 : -0.0465e-9) + bin(CH_B4_uc1, mobmod == 1 ? -0.056 : -0.056e-9) * tr1;
  O(u0temp) = u0 * std::pow(tr, bin(CH_B4_ute, -1.5));
  O(eu) = bin(CH_B4_eu, type > 0 ? 1.67 : 1.0);
  O(vsattemp) = bin(CH_B4_vsat, 8e4) - bin(CH_B4_at, 3.3e4) * tr1;
  const double a0 = bin(CH_B4_a0, 1.0);
  O(a0) = a0; O(agsa0) = bin(CH_B4_ags, 0) * a0; O(a1) = bin(CH_B4_a1, 0); O(a2) = bin(CH_B4_a2, 1.0);
  O(b0term) = bin(CH_B4_b0, 0) / (weff + bin(CH_B4_b1, 0));
  O(keta) = bin(CH_B4_keta, -0.047); O(xj) = xj; O(dwg) = bin(CH_B4_dwg, 0); O(dwb) = bin(CH_B4_dwb, 0);
  {
    const double prt = bin(CH_B4_prt, 0), pww = std::pow(weffCJ * 1e6, bin(CH_B4_wr, 1.0)) * nf;
    double r0 = (bin(CH_B4_rdsw, 200.0) + prt * tr1) * nf / pww, rmin = (par(CH_B4_rdswmin, 0) + prt * tr1) * nf / pww;
    O(rds0h) = 0.5 * (r0 < 0 ? 0 : r0); O(rdswmin) = rmin < 0 ? 0 : rmin;
  }
  O(prwg) = bin(CH_B4_prwg, 1.0); O(prwb) = bin(CH_B4_prwb, 0); O(delta) = bin(CH_B4_delta, 0.01);
  O(pclmlitl) = bin(CH_B4_pclm, 1.3) * litl;  // pclm*litl; pclm <= MIN_EXP encoded as 0
  if (bin(CH_B4_pclm, 1.3) <= MIN_EXP) O(pclmlitl) = 0.0;
  O(pdiblb) = bin(CH_B4_pdiblcb, 0);
  { const double fp = bin(CH_B4_fprout, 0); O(fproutL) = fp <= 0 ? 0.0 : fp * std::sqrt(leff); }
  O(pdits) = bin(CH_B4_pdits, 0); O(pditsd) = bin(CH_B4_pditsd, 0); O(pditslL) = 1.0 + par(CH_B4_pditsl, 0) * leff;
  O(pscbe1l) = bin(CH_B4_pscbe1, 4.24e8) * litl; O(pscbe2) = bin(CH_B4_pscbe2, 1e-5); O(pvag) = bin(CH_B4_pvag, 0);
  { const double al = bin(CH_B4_alpha0, 0) + bin(CH_B4_alpha1, 0) * leff; O(alphaL) = al <= 0 ? 0.0 : al / leff; }
  O(beta0) = bin(CH_B4_beta0, 0);
  {
    const double ag = bin(CH_B4_agidl, 0), bg = bin(CH_B4_bgidl, 2.3e9), cg = bin(CH_B4_cgidl, 0.5);
    O(agidlW) = (ag > 0 && bg > 0 && cg > 0) ? ag * weffCJ * nf : 0.0;
    O(bgidl) = bg; O(cgidl) = cg; O(egidl) = bin(CH_B4_egidl, 0.8); O(toxe3) = 3.0 * toxe;
  }
  // charge model
  O(xpart) = par(CH_B4_xpart, 0);
  const double cgsl = bin(CH_B4_cgsl, 0), cgdl = bin(CH_B4_cgdl, 0);
  const double cf = has(CH_B4_cf) ? bin(CH_B4_cf, 0) : 2.0 * epsrox * EPS0 / PI * std::log(1.0 + 0.4e-6 / toxe);
  const bool dlcOK = has(CH_B4_dlc) && dlc0 > 0;
  const double cgdo = has(CH_B4_cgdo) ? mp[CH_B4_cgdo] : (dlcOK ? dlc0 * coxe - cgdl : 0.6 * xj * coxe);
  const double cgso = has(CH_B4_cgso) ? mp[CH_B4_cgso] : (dlcOK ? dlc0 * coxe - cgsl : 0.6 * xj * coxe);
  const double cgbo = has(CH_B4_cgbo) ? mp[CH_B4_cgbo] : 2.0 * dwc0 * coxe;
  O(cgdo) = (cgdo + cf) * weffCV * nf; O(cgso) = (cgso + cf) * weffCV * nf; O(cgbo) = cgbo * leffCV * nf;
  O(cgslW) = cgsl * weffCV * nf; O(cgdlW) = cgdl * weffCV * nf;
  O(ckappas) = bin(CH_B4_ckappas, 0.6);
  O(ckappad) = has(CH_B4_ckappad) ? bin(CH_B4_ckappad, 0.6) : out[B4I_ckappas];
  O(abulkCVfactor) = 1.0 + std::pow(bin(CH_B4_clc, 1e-7) / leffCV, bin(CH_B4_cle, 0.6));
  O(acde) = bin(CH_B4_acde, 1.0) * std::pow(ndep / 2e16, -0.25);
  O(moinVtm) = bin(CH_B4_moin, 15.0) * vtm;
  O(noff) = bin(CH_B4_noff, 1.0); O(voffcv) = bin(CH_B4_voffcv, 0);
  O(CoxWL) = coxe * weffCV * leffCV * nf; O(toxp8) = 1e8 * toxp;
  // junctions
  {
    double jss = par(CH_B4_jss, 1e-4), jsws = par(CH_B4_jsws, 0), jswgs = par(CH_B4_jswgs, 0);
    double jsd = par(CH_B4_jsd, jss), jswd = par(CH_B4_jswd, jsws), jswgd = par(CH_B4_jswgd, jswgs);
    const double njs = par(CH_B4_njs, 1.0), njd = par(CH_B4_njd, njs);
    const double xtis = par(CH_B4_xtis, 3.0), xtid = par(CH_B4_xtid, xtis);
    if (dT != 0.0) {
      const double e0 = Eg0 / vtm0 - Eg / vtm, lt = std::log(tr);
      const double fs = std::exp((e0 + xtis * lt) / njs), fd = std::exp((e0 + xtid * lt) / njd);
      jss *= fs; jsws *= fs; jswgs *= fs; jsd *= fd; jswd *= fd; jswgd *= fd;
    }
    auto ct = [&](double c, double tc) { const double f = 1.0 + tc * dT; return f > 0 ? c * f : 0.0; };
    auto pt = [&](double p, double tp) { const double r = p - tp * dT; return r < 0.01 ? 0.01 : r; };
    const double tcj = par(CH_B4_tcj, 0), tcjsw = par(CH_B4_tcjsw, 0), tcjswg = par(CH_B4_tcjswg, 0);
    const double tpb = par(CH_B4_tpb, 0), tpbsw = par(CH_B4_tpbsw, 0), tpbswg = par(CH_B4_tpbswg, 0);
    const double cjs = par(CH_B4_cjs, 5e-4), cjd = par(CH_B4_cjd, cjs);
    const double cjsws = par(CH_B4_cjsws, 5e-10), cjswd = par(CH_B4_cjswd, cjsws);
    const double cjswgs = par(CH_B4_cjswgs, cjsws), cjswgd = par(CH_B4_cjswgd, cjswgs);
    const double pbs = par(CH_B4_pbs, 1.0), pbd = par(CH_B4_pbd, pbs), pbsws = par(CH_B4_pbsws, 1.0);
    const double pbswd = par(CH_B4_pbswd, pbsws), pbswgs = par(CH_B4_pbswgs, pbsws), pbswgd = par(CH_B4_pbswgd, pbswgs);
    O(mjs) = par(CH_B4_mjs, 0.5); O(mjd) = par(CH_B4_mjd, out[B4I_mjs]);
    O(mjsws) = par(CH_B4_mjsws, 0.33); O(mjswd) = par(CH_B4_mjswd, out[B4I_mjsws]);
    O(mjswgs) = par(CH_B4_mjswgs, out[B4I_mjsws]); O(mjswgd) = par(CH_B4_mjswgd, out[B4I_mjswgs]);
    O(PhiBS) = pt(pbs, tpb); O(PhiBD) = pt(pbd, tpb); O(PhiBSWS) = pt(pbsws, tpbsw); O(PhiBSWD) = pt(pbswd, tpbsw);
    O(PhiBSWGS) = pt(pbswgs, tpbswg); O(PhiBSWGD) = pt(pbswgd, tpbswg);
    // geoMod 0 diffusion geometry (isolated end diffusions, shared internal ones)
    const double dmcg = par(CH_B4_dmcg, 0), dmci = par(CH_B4_dmci, dmcg);
    const double Piso = 2.0 * (dmcg + dmci) + weffCJ, Aiso = (dmcg + dmci) * weffCJ, Psha = 2.0 * dmcg, Asha = dmcg * weffCJ;
    double eS, iS, eD, iD;
    if (((long)nf) % 2) { eS = eD = 1.0; iS = iD = (nf - 1.0) / 2.0; } else { eD = 0.0; iD = nf / 2.0; eS = 2.0; iS = nf / 2.0 - 1.0; }
    auto g = [&](int kpar) { return !std::isnan(ip[kpar]); };
    const double As = g(CH_MOS_AS) ? ip[CH_MOS_AS] : eS * Aiso + iS * Asha, Ad = g(CH_MOS_AD) ? ip[CH_MOS_AD] : eD * Aiso + iD * Asha;
    double Ps = g(CH_MOS_PS) ? (permod == 0 ? ip[CH_MOS_PS] : ip[CH_MOS_PS] - weffCJ * nf) : eS * Piso + iS * Psha;
    double Pd = g(CH_MOS_PD) ? (permod == 0 ? ip[CH_MOS_PD] : ip[CH_MOS_PD] - weffCJ * nf) : eD * Piso + iD * Psha;
    if (Ps < 0) Ps = 0;
    if (Pd < 0) Pd = 0;
    const double Isbs = As * jss + Ps * jsws + weffCJ * nf * jswgs, Isbd = Ad * jsd + Pd * jswd + weffCJ * nf * jswgd;
    O(Isbs) = Isbs; O(Isbd) = Isbd; O(Nvtms) = vtm * njs; O(Nvtmd) = vtm * njd;
    const double ijs = par(CH_B4_ijthsfwd, 0.1), ijd = par(CH_B4_ijthdfwd, ijs);
    if (Isbs > 0) { O(vjsmFwd) = vtm * njs * std::log(ijs / Isbs + 1.0); O(IVjsmFwd) = Isbs * std::exp(out[B4I_vjsmFwd] / (vtm * njs)); }
    if (Isbd > 0) { O(vjdmFwd) = vtm * njd * std::log(ijd / Isbd + 1.0); O(IVjdmFwd) = Isbd * std::exp(out[B4I_vjdmFwd] / (vtm * njd)); }
    O(czbs) = ct(cjs, tcj) * As; O(czbssw) = ct(cjsws, tcjsw) * Ps; O(czbsswg) = ct(cjswgs, tcjswg) * weffCJ * nf;
    O(czbd) = ct(cjd, tcj) * Ad; O(czbdsw) = ct(cjswd, tcjsw) * Pd; O(czbdswg) = ct(cjswgd, tcjswg) * weffCJ * nf;
  }
#undef O
  return CH_OK;
}

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// Device side.
//
// fp64 division and square root dominate the instruction count of a compact model; the IEEE
// sequences hipcc emits cost ~11 / ~15 VALU instructions.  frcp/fsqrt use the hardware seeds
// (v_rcp_f64, v_rsq_f64) plus Newton steps: <= 1-2 ulp, which is far inside the 1e-10 parity bar.
// v_rcp_f64 is good to 4.6e-8 relative on gfx950 (scripts/rcp_accuracy.hip); one cubically convergent correction
// r·(1 + e + e²), e = 1 − x·r, brings it to the rounding limit with three FMAs
CH_D double frcp(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  const double e = fma(-x, r, 1.0);
  return fma(r, fma(e, e, e), r);
}
CH_D double fsqrt(double x) {  // x > 0
  double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  double r = fma(-h, g, 0.5);
  g = fma(g, r, g); h = fma(h, r, h);
  r = fma(-h, g, 0.5);
  g = fma(g, r, g); h = fma(h, r, h);
  g = fma(fma(-g, g, x), h, g);
  return g;
}

// value + N partial derivatives.  N = 3: (d/dVgs', d/dVds', d/dVbs') in one lane.
// N = 1: one partial per lane, four lanes per instance (the fourth carries a zero seed).
//
// S says at compile time, three bits per partial, which partials EXIST (default: all of them).  A partial that does not exist is an
// exact zero; it is neither stored (p holds the existing ones, in order) nor computed.  Every operator returns the union of its
// operands' sets and computes an existing partial by the expression the dense form uses with the structurally zero terms taken out
// and nothing else touched: fma(a.p, b.v, a.v*b.p) is a.p*b.v when b.p does not exist and a.v*b.p when a.p does not, a sum with
// such a term is the other term.  fma(x, y, +-0) and x*y round the same product once, so the values are those of the dense form
// but for the sign of an exact zero (and a 0*inf NaN of the dense form, which becomes finite).
//
// hipcc contracts a*b + c across the inlined operators, so "nothing else touched" needs the five states below: they follow what
// the compiler makes of the DENSE form, in which the zeros are there.
//   * a product that stands where the dense form has an fma must not be contracted into an add that follows: dn::mulr;
//   * PX marks a partial that is a contractable product right now (x.p*c of operator*(DN, double), chain, recip, operator/).  Where
//     the dense form adds a zero that the compiler cannot fold away (x + 0, x - (-0), 0 - x, or a zero it only knows at run time),
//     product and add contract to fma(x, y, 0): one rounding, closed to further contraction.  Dropping that add would hand the bare
//     product to the NEXT add and save its rounding, so there the zero is still added; it costs nothing, the multiply becomes
//     the fma.  Where the compiler folds the add (x + (-0), x - 0, (-0) - x) the dense form keeps the bare product too, and so
//     does this one.  ZP / ZN / ZR (a literal +0, a literal -0, a zero that went through a multiplication) are what decides it.
//     A partial that is not a product (PR) simply loses its add.
// A conversion to a wider set (the explicit widening where two control-flow paths join) stores the zeros and forgets PX: across a
// join the optimiser has been seen to contract nothing.  Straight-line code keeps its intermediates `auto`.
// None of ZP / ZN / ZR / PX is a property of the arithmetic: they describe how the hipcc this was written against contracts the
// dense form, and the bit goldens (tests/test_gpu_b4_bits.py, tests/test_gpu_lockstep_bits.py) are their sole proof.  They buy
// equality with the recorded dense build and nothing else.  When a compiler upgrade moves the dense form's bits too, re-record the
// goldens and collapse the states to exists / absent (mulr -> a plain product, no kept `+ 0.0`): the values then differ from the
// dense form's by roundings of partials, far inside the 1e-10 stamp tolerance of tests/test_gpu_bsim4_cards.py.
namespace dn {
enum : unsigned { ZP = 0, ZN = 1, ZR = 2, PR = 3, PX = 4 };
constexpr unsigned st(unsigned s, int i) { return (s >> (3 * i)) & 7u; }
constexpr bool has(unsigned s, int i) { return st(s, i) >= PR; }
constexpr int slot(unsigned s, int i) { int c = 0; for (int j = 0; j < i; ++j) c += has(s, j) ? 1 : 0; return c; }
constexpr unsigned all(int n, unsigned k) { unsigned s = 0; for (int i = 0; i < n; ++i) s |= k << (3 * i); return s; }
constexpr unsigned mask(unsigned s, int n) { unsigned m = 0; for (int i = 0; i < n; ++i) m |= has(s, i) ? 1u << i : 0u; return m; }
constexpr unsigned from_mask(unsigned m, int n) { unsigned s = 0; for (int i = 0; i < n; ++i) s |= (((m >> i) & 1u) ? PR : ZR) << (3 * i); return s; }
constexpr unsigned neg1(unsigned a) { return a == ZP ? ZN : (a == ZN ? ZP : a); }
constexpr unsigned add1(unsigned a, unsigned b) {
  if (a >= PR && b >= PR) return PR;
  if (a >= PR) return b == ZN ? a : PR;
  if (b >= PR) return a == ZN ? b : PR;
  return (a == ZR || b == ZR) ? ZR : ((a == ZN && b == ZN) ? ZN : ZP);
}
constexpr unsigned sub1(unsigned a, unsigned b) {
  if (a >= PR && b >= PR) return PR;
  if (a >= PR) return b == ZP ? a : PR;
  if (b >= PR) return a == ZN ? b : PR;
  return (a == ZR || b == ZR) ? ZR : ((a == ZN && b == ZP) ? ZN : ZP);
}
constexpr unsigned scl1(unsigned a, unsigned) { return a >= PR ? PX : ZR; }                       // x.p * c
constexpr unsigned mul1(unsigned a, unsigned b) { return (a >= PR || b >= PR) ? PR : ZR; }        // fma(a.p, b.v, a.v*b.p)
constexpr unsigned div1(unsigned a, unsigned b) { return (a >= PR || b >= PR) ? PX : ZR; }        // fma(-q, b.p, a.p) * r
constexpr unsigned lift(unsigned (*f)(unsigned, unsigned), unsigned a, unsigned b, int n) {
  unsigned s = 0; for (int i = 0; i < n; ++i) s |= f(st(a, i), st(b, i)) << (3 * i); return s;
}
constexpr unsigned neg(unsigned a, int n) { unsigned s = 0; for (int i = 0; i < n; ++i) s |= neg1(st(a, i)) << (3 * i); return s; }
CH_D double mulr(double x, double y) {
#pragma clang fp contract(off)
  return x * y;
}
}  // namespace dn
template <int N, unsigned S = dn::all(N, dn::PR)>
struct DN {
  static constexpr int n = N, cnt = dn::slot(S, N);
  static constexpr unsigned state = S, mask = dn::mask(S, N);
  double v, p[cnt ? cnt : 1];
  DN() = default;
  // widening: the partials of a, its zeros where it has none
  template <unsigned S2>
  CH_D DN(const DN<N, S2>& a) {
    v = a.v;
    static_assert(ok_from(S2), "a conversion only widens");
    for (int i = 0; i < N; ++i) if (dn::has(S, i)) p[dn::slot(S, i)] = a.get(i);
  }
  static constexpr bool ok_from(unsigned s2) {
    for (int i = 0; i < N; ++i) {
      const unsigned t = dn::st(S, i), f = dn::st(s2, i);
      if (!(t == dn::PR || (t == dn::ZR && f < dn::PR) || t == f)) return false;
    }
    return true;
  }
  CH_D double get(int i) const { return dn::has(S, i) ? p[dn::slot(S, i)] : (dn::st(S, i) == dn::ZN ? -0.0 : 0.0); }
};
// a constant with its zero partials stored (the dense form), and one that has none
template <int N> CH_D DN<N> mkd(double v) { DN<N> r; r.v = v; for (int i = 0; i < N; ++i) r.p[i] = 0.0; return r; }
template <int N> CH_D DN<N, dn::all(N, dn::ZP)> cstd(double v) { DN<N, dn::all(N, dn::ZP)> r; r.v = v; return r; }
// the seed of direction I: d/dI = 1, nothing else
template <int N, int I> CH_D DN<N, dn::PR << (3 * I)> seed(double v) { DN<N, dn::PR << (3 * I)> r; r.v = v; r.p[0] = 1.0; return r; }
#define CH_DN_EACH(SR) for (int i = 0; i < N; ++i) if (dn::has(SR, i))
template <int N, unsigned SA, unsigned SB> CH_D DN<N, dn::lift(dn::add1, SA, SB, N)> operator+(DN<N, SA> a, DN<N, SB> b) {
  constexpr unsigned SR = dn::lift(dn::add1, SA, SB, N);
  DN<N, SR> r; r.v = a.v + b.v;
  CH_DN_EACH(SR) {
    double& o = r.p[dn::slot(SR, i)];
    const unsigned sa = dn::st(SA, i), sb = dn::st(SB, i);
    if (sa >= dn::PR && sb >= dn::PR) o = a.get(i) + b.get(i);
    else if (sa >= dn::PR) o = (sa == dn::PX && sb != dn::ZN) ? a.get(i) + 0.0 : a.get(i);
    else o = (sb == dn::PX && sa != dn::ZN) ? b.get(i) + 0.0 : b.get(i);
  }
  return r;
}
template <int N, unsigned SA, unsigned SB> CH_D DN<N, dn::lift(dn::sub1, SA, SB, N)> operator-(DN<N, SA> a, DN<N, SB> b) {
  constexpr unsigned SR = dn::lift(dn::sub1, SA, SB, N);
  DN<N, SR> r; r.v = a.v - b.v;
  CH_DN_EACH(SR) {
    double& o = r.p[dn::slot(SR, i)];
    const unsigned sa = dn::st(SA, i), sb = dn::st(SB, i);
    if (sa >= dn::PR && sb >= dn::PR) o = a.get(i) - b.get(i);
    else if (sa >= dn::PR) o = (sa == dn::PX && sb != dn::ZP) ? a.get(i) + 0.0 : a.get(i);
    else o = (sb == dn::PX && sa != dn::ZN) ? 0.0 - b.get(i) : -b.get(i);
  }
  return r;
}
template <int N, unsigned S> CH_D DN<N, dn::neg(S, N)> operator-(DN<N, S> a) { DN<N, dn::neg(S, N)> r; r.v = -a.v; for (int i = 0; i < a.cnt; ++i) r.p[i] = -a.p[i]; return r; }
template <int N, unsigned S> CH_D DN<N, S> operator+(DN<N, S> a, double b) { a.v += b; return a; }
template <int N, unsigned S> CH_D DN<N, S> operator+(double b, DN<N, S> a) { a.v += b; return a; }
template <int N, unsigned S> CH_D DN<N, S> operator-(DN<N, S> a, double b) { a.v -= b; return a; }
template <int N, unsigned S> CH_D DN<N, dn::neg(S, N)> operator-(double b, DN<N, S> a) { DN<N, dn::neg(S, N)> r; r.v = b - a.v; for (int i = 0; i < a.cnt; ++i) r.p[i] = -a.p[i]; return r; }
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> operator*(DN<N, S> a, double b) { DN<N, dn::lift(dn::scl1, S, S, N)> r; r.v = a.v * b; for (int i = 0; i < a.cnt; ++i) r.p[i] = a.p[i] * b; return r; }
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> operator*(double b, DN<N, S> a) { return a * b; }
template <int N, unsigned SA, unsigned SB> CH_D DN<N, dn::lift(dn::mul1, SA, SB, N)> operator*(DN<N, SA> a, DN<N, SB> b) {
  constexpr unsigned SR = dn::lift(dn::mul1, SA, SB, N);
  DN<N, SR> r; r.v = a.v * b.v;
  CH_DN_EACH(SR) {
    double& o = r.p[dn::slot(SR, i)];
    if (dn::has(SA, i) && dn::has(SB, i)) o = fma(a.get(i), b.v, a.v * b.get(i));
    else if (dn::has(SA, i)) o = dn::mulr(a.get(i), b.v);
    else o = dn::mulr(a.v, b.get(i));
  }
  return r;
}
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> recip(DN<N, S> a) { const double r = frcp(a.v), m = -r * r; DN<N, dn::lift(dn::scl1, S, S, N)> o; o.v = r; for (int i = 0; i < a.cnt; ++i) o.p[i] = a.p[i] * m; return o; }
template <int N, unsigned SA, unsigned SB> CH_D DN<N, dn::lift(dn::div1, SA, SB, N)> operator/(DN<N, SA> a, DN<N, SB> b) {
  constexpr unsigned SR = dn::lift(dn::div1, SA, SB, N);
  const double r = frcp(b.v), q = a.v * r;
  DN<N, SR> o; o.v = q;
  CH_DN_EACH(SR) {
    double& x = o.p[dn::slot(SR, i)];
    if (dn::has(SA, i) && dn::has(SB, i)) x = fma(-q, b.get(i), a.get(i)) * r;
    else if (dn::has(SA, i)) x = a.get(i) * r;
    else x = dn::mulr(-q, b.get(i)) * r;
  }
  return o;
}
#undef CH_DN_EACH
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> operator/(DN<N, S> a, double b) { return a * frcp(b); }
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> operator/(double a, DN<N, S> b) { return recip(b) * a; }
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> chain(DN<N, S> a, double f, double fp) { DN<N, dn::lift(dn::scl1, S, S, N)> r; r.v = f; for (int i = 0; i < a.cnt; ++i) r.p[i] = a.p[i] * fp; return r; }
template <int N, unsigned S> CH_D DN<N, dn::lift(dn::scl1, S, S, N)> dsqrt(DN<N, S> a) { const double s = fsqrt(a.v); return chain(a, s, 0.5 * frcp(s)); }
// ---- where the polynomial coefficients of fexp / flog come from ----
// An fp64 literal has no cheap home on gfx9: a VOP3 instruction carries none, so every use costs two 32-bit moves, and with one
// wavefront per SIMD (the device-resident stepper) each of them is a full issue turn.  The 25 constants below are therefore
// read from a source K: KLit gives them as literals (every kernel but the device-resident stepper: what the compiler did before),
// KLds reads them from a table the workgroup keeps in LDS (kpool_fill), two per ds_read_b128 at a wave-uniform address, straight
// into the registers the FMA chain accumulates in.  They are plain reads of a table whose size the compiler knows: it may merge,
// hoist and speculate them like the literals they replace.  Reads it cannot see through (volatile, or an address passed through an
// empty asm to keep every inlined copy's reads apart) were tried and cost more than they saved: the optimiser then no longer
// treats the inlined copies alike, and the evaluation grew by a thousand instructions (profiles/r06_notes.md).  The constants a
// function needs at once (range reduction of fexp, the mantissa threshold of flog) come from the table too: measured, not assumed
// (the reads are hoisted far enough; evaluation stamp 24.07 k -> 23.87 k cycles).  +-inf, 1024 and -1075 stay literals: their low
// word is zero, one move each.
enum { KP_EXP = 0, KP_LOG = 10, KP_PRE = 22, KP_COUNT = 26 };
#define CH_KPOOL_VALUES                                                                                                        \
  /* fexp: c11 .. c2 of the library polynomial */                                                                              \
  0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22, 0x1.71dee623fde64p-19, 0x1.a01997c89e6b0p-16, 0x1.a01a014761f6ep-13,           \
  0x1.6c16c1852b7b0p-10, 0x1.1111111122322p-7, 0x1.55555555502a1p-5, 0x1.5555555555511p-3, 0x1.000000000000bp-1,               \
  /* flog: 1/19 .. 1/3, the two parts of ln 2, sqrt(1/2); then fexp's 1/ln 2 and the two parts of ln 2 */                      \
  1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0, 1.0 / 5.0, 1.0 / 3.0,                      \
  6.93147180369123816490e-01, 1.90821492927058770002e-10, 0.70710678118654752440,                                             \
  0x1.71547652b82fep+0, 0x1.62e42fefa39efp-1, 0x1.abc9e3b39803fp-56, 0.0
struct KLit {
  template <int I> CH_D void pair(double& a, double& b) const { constexpr double t[KP_COUNT] = {CH_KPOOL_VALUES}; a = t[I]; b = t[I + 1]; }
};
typedef double kp_d2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(3))) kp_d2* kp_lds_ptr;
struct KLds {
  kp_lds_ptr p;   // 16-byte aligned table of KP_COUNT doubles in LDS
  template <int I> CH_D void pair(double& a, double& b) const { static_assert(I % 2 == 0, "pairs are 16-byte aligned"); const kp_d2 v = p[I / 2]; a = v.x; b = v.y; }
};
// every thread of the workgroup calls this before the first evaluation, with a barrier between it and the first use
CH_D KLds kpool_fill(double* lds_table, int tid) {
  constexpr double t[KP_COUNT] = {CH_KPOOL_VALUES};
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < KP_COUNT; ++i) v = (tid == i) ? t[i] : v;
  if (tid < KP_COUNT) lds_table[tid] = v;
  return KLds{(kp_lds_ptr)(__attribute__((address_space(3))) double*)lds_table};
}

// e^x, bit for bit the library's exp on gfx950 (tests/test_gpu_fexp_bits.py): the same operations in the same order with the same
// constants and range selects as the sequence hipcc inlines for exp(double) — n = rint(x / ln 2), t = x − n·ln2_hi − n·ln2_lo,
// a degree-11 polynomial in t by Horner's rule, ldexp by n, +inf above 1024 and 0 below −1075 — written out so that its
// coefficients can come from K.
template <class K>
CH_D double fexp(double x, const K k) {
#if defined(__HIP_DEVICE_COMPILE__)
  double c11, c10, c9, c8, c7, c6, c5, c4, c3, c2;
  k.template pair<KP_EXP + 0>(c11, c10); k.template pair<KP_EXP + 2>(c9, c8); k.template pair<KP_EXP + 4>(c7, c6);
  k.template pair<KP_EXP + 6>(c5, c4); k.template pair<KP_EXP + 8>(c3, c2);
  double il2, l2h, l2l, pd;
  k.template pair<KP_PRE + 0>(il2, l2h); k.template pair<KP_PRE + 2>(l2l, pd);
  const double dn = __builtin_rint(x * il2);
  double t = fma(-dn, l2h, x);
  t = fma(-dn, l2l, t);
  double p = fma(t, c11, c10);
  p = fma(t, p, c9); p = fma(t, p, c8); p = fma(t, p, c7); p = fma(t, p, c6); p = fma(t, p, c5); p = fma(t, p, c4);
  p = fma(t, p, c3); p = fma(t, p, c2); p = fma(t, p, 1.0); p = fma(t, p, 1.0);
  double z = __builtin_ldexp(p, (int)dn);
  z = x > 1024.0 ? __builtin_inf() : z;
  z = x < -1075.0 ? 0.0 : z;
  return z;
#else
  return exp(x);
#endif
}
CH_D double fexp(double x) { return fexp(x, KLit{}); }
template <int N, unsigned S, class K> CH_D auto dexp(DN<N, S> a, const K k) { const double e = fexp(a.v, k); return chain(a, e, e); }
template <int N, unsigned S> CH_D auto dexp(DN<N, S> a) { return dexp(a, KLit{}); }
// Natural logarithm for positive finite normal arguments (every use below: junction terms, smoothing functions and
// mobility powers).  x = m·2^e with m in [sqrt(1/2), sqrt(2)); s = (m−1)/(m+1); ln m = 2s(1 + s²/3 + … + s¹⁸/19),
// |s| ≤ 0.1716 so the truncation error is 2e-17.  ≈ 28 instructions against 118 for the library log on gfx950
// (76 of them fp64); 0, negative, NaN and +inf arguments are handled by a final selection.
template <class K>
CH_D double flog(double x, const K k) {
#if defined(__HIP_DEVICE_COMPILE__)
  double l19, l17, l15, l13, l11, l9, l7, l5, l3, ln2h, ln2l, pad;   // pad: sqrt(1/2)
  k.template pair<KP_LOG + 0>(l19, l17); k.template pair<KP_LOG + 2>(l15, l13); k.template pair<KP_LOG + 4>(l11, l9);
  k.template pair<KP_LOG + 6>(l7, l5); k.template pair<KP_LOG + 8>(l3, ln2h); k.template pair<KP_LOG + 10>(ln2l, pad);
  double m = __builtin_amdgcn_frexp_mant(x);          // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool lo = m < pad;
  m = lo ? 2.0 * m : m;
  e = lo ? e - 1 : e;
  const double s = (m - 1.0) * frcp(m + 1.0);
  const double z = s * s;
  double p = l19;
  p = fma(p, z, l17); p = fma(p, z, l15); p = fma(p, z, l13); p = fma(p, z, l11);
  p = fma(p, z, l9); p = fma(p, z, l7); p = fma(p, z, l5); p = fma(p, z, l3);
  const double lm = fma(2.0 * s, p * z, 2.0 * s);
  const double de = (double)e;
  const double r = fma(de, ln2h, fma(de, ln2l, lm));
  // special cases by selection (no branch): 0 -> -inf, negative / NaN -> NaN, +inf -> +inf
  return (x > 0.0 && x < __builtin_inf()) ? r : (x == 0.0 ? -__builtin_inf() : (x > 0.0 ? x : __builtin_nan("")));
#else
  return log(x);
#endif
}
CH_D double flog(double x) { return flog(x, KLit{}); }
template <int N, unsigned S, class K> CH_D auto dlog(DN<N, S> a, const K k) { return chain(a, flog(a.v, k), frcp(a.v)); }
template <int N, unsigned S> CH_D auto dlog(DN<N, S> a) { return chain(a, flog(a.v), frcp(a.v)); }

// smooth SCE factor e^x/((e^x-1)^2 + 2 e^x MIN_EXP)
// (two paths join here: the result is widened to the partials of x, the constant's zeros stored)
template <int N, unsigned S, class K> CH_D DN<N, dn::from_mask(dn::mask(S, N), N)> d_sce(DN<N, S> x, const K kc) {
  if (x.v < k::EXP_TH) {
    const auto e = dexp(x, kc), m1 = e - 1.0;
    return e / (m1 * m1 + e * (2.0 * k::MIN_EXP));
  }
  return cstd<N>(1.0 / (k::MAX_EXP - 2.0));
}

struct B4Col {
  // One packed column per class, parameters contiguous ([column][B4I_COUNT]): the ~140 values one
  // lane needs sit in 9 consecutive cache lines, and the 8 classes of a DFF block fit in L1.
  const double* p;  // base of this lane's column
  CH_D double operator[](int i) const { return p[i]; }
};
CH_D B4Col b4_col(const double* table, long col) { return B4Col{table + col * (long)B4I_COUNT}; }

// ---- values that depend on the packed column alone ----
// The reciprocals the model takes of card values (or of a value formed from card values alone), in order of use: the front end,
// Vgsteff, mobility, the channel, the output resistance, GIDL, the charges; then the junctions of the source side, of the drain
// side, and the overlaps.  b4_derive is their ONE definition.  Where the model gets them from is a source D, like K for the
// polynomial coefficients:
//   B4DHere  computed at the use by b4_derive (every kernel but the device-resident stepper: what the code did before);
//   B4DTab   read from a table of B4D_STRIDE doubles per class that b4_derive filled once per transient (tran_persistent_kernel:
//            a lane keeps its device and its class for the whole transient, so the Newton loop need not divide by card values).
// Both give the same bits: the same function of the same column.
enum B4DIdx {
  B4D_itoxe, B4D_icoxe, B4D_iLeff, B4D_isqrtPhi, B4D_ipolyT1, B4D_icdep0, B4D_iu0temp, B4D_ivsat, B4D_itoxp8, B4D_ipclmlitl,
  B4D_ithetaRout, B4D_ipdits, B4D_itoxe3, B4D_ik1ox, B4D_iDen,
  B4D_iNvtms, B4D_iNvtmd,
  B4D_iPhiBS, B4D_iPhiBSWS, B4D_iPhiBSWGS, B4D_i1mjs, B4D_i1mjsws, B4D_i1mjswgs,
  B4D_iPhiBD, B4D_iPhiBSWD, B4D_iPhiBSWGD, B4D_i1mjd, B4D_i1mjswd, B4D_i1mjswgd,
  B4D_ickappad, B4D_ickappas, B4D_COUNT
};
constexpr int B4D_STRIDE = 32;
static_assert(B4D_COUNT <= B4D_STRIDE, "one table row per class");
CH_D double b4_derive(const B4Col P, int i) {
  switch (i) {
    case B4D_itoxe: return frcp(P[B4I_toxe]);
    case B4D_icoxe: return frcp(P[B4I_coxe]);
    case B4D_iLeff: return frcp(P[B4I_leff]);
    case B4D_isqrtPhi: return frcp(P[B4I_sqrtPhi]);
    case B4D_ipolyT1: return frcp(P[B4I_polyT1]);
    case B4D_icdep0: return frcp(P[B4I_cdep0]);
    case B4D_iu0temp: return frcp(P[B4I_u0temp]);
    case B4D_ivsat: return frcp(P[B4I_vsattemp]);
    case B4D_itoxp8: return frcp(P[B4I_toxp8]);
    case B4D_ipclmlitl: return frcp(P[B4I_pclmlitl]);
    case B4D_ithetaRout: return frcp(P[B4I_thetaRout]);
    case B4D_ipdits: return frcp(P[B4I_pdits]);
    case B4D_itoxe3: return frcp(P[B4I_toxe3]);
    case B4D_ik1ox: return frcp(P[B4I_k1ox]);
    case B4D_iDen: { const double k1ox = P[B4I_k1ox]; return frcp(k1ox <= 0.0 ? 0.25 * P[B4I_moinVtm] : P[B4I_moinVtm] * k1ox * k1ox); }
    case B4D_iNvtms: return frcp(P[B4I_Nvtms]);
    case B4D_iNvtmd: return frcp(P[B4I_Nvtmd]);
    case B4D_iPhiBS: return frcp(P[B4I_PhiBS]);
    case B4D_iPhiBSWS: return frcp(P[B4I_PhiBSWS]);
    case B4D_iPhiBSWGS: return frcp(P[B4I_PhiBSWGS]);
    case B4D_i1mjs: return frcp(1.0 - P[B4I_mjs]);
    case B4D_i1mjsws: return frcp(1.0 - P[B4I_mjsws]);
    case B4D_i1mjswgs: return frcp(1.0 - P[B4I_mjswgs]);
    case B4D_iPhiBD: return frcp(P[B4I_PhiBD]);
    case B4D_iPhiBSWD: return frcp(P[B4I_PhiBSWD]);
    case B4D_iPhiBSWGD: return frcp(P[B4I_PhiBSWGD]);
    case B4D_i1mjd: return frcp(1.0 - P[B4I_mjd]);
    case B4D_i1mjswd: return frcp(1.0 - P[B4I_mjswd]);
    case B4D_i1mjswgd: return frcp(1.0 - P[B4I_mjswgd]);
    case B4D_ickappad: return frcp(P[B4I_ckappad]);
    case B4D_ickappas: return frcp(P[B4I_ckappas]);
  }
  return 0.0;
}
struct B4DHere {
  CH_D double get(const B4Col P, int i) const { return b4_derive(P, i); }
};
struct B4DTab {
  const double* d;   // this lane's row of the table
  CH_D double get(const B4Col, int i) const { return d[i]; }
};

// junction diode current and conductance (dioMod 1) incl. gmin
// (iNvtm: the entry of B4DIdx that holds 1/Nvtm of this junction)
template <class K, class DS>
CH_D void diode(const K kc, const DS ds, const B4Col P, int iNvtm, double vb, double Is, double vjm, double IVjm, double gmin, double& i, double& g) {
  if (Is <= 0.0) { i = gmin * vb; g = gmin; return; }
  const double iN = ds.get(P, iNvtm);
  if (vb <= vjm) {
    const double t = vb * iN;
    if (t < -k::EXP_TH) { i = Is * (k::MIN_EXP - 1.0) + gmin * vb; g = gmin; }
    else { const double e = fexp(t, kc); i = Is * (e - 1.0) + gmin * vb; g = Is * e * iN + gmin; }
  } else {
    const double s = IVjm * iN;
    i = IVjm - Is + s * (vb - vjm) + gmin * vb; g = s + gmin;
  }
}
// junction depletion charge and capacitance
// (d0: the first of this side's six entries of B4DIdx: 1/pb, 1/pbsw, 1/pbswg, 1/(1 - mj), 1/(1 - mjsw), 1/(1 - mjswg))
template <class K, class DS>
CH_D void junction(const K kc, const DS ds, const B4Col P, int d0, double vb, double cz, double czsw, double czswg, double pb, double pbsw, double pbswg, double mj,
                   double mjsw, double mjswg, double& q, double& c) {
  if (vb < 0.0) {
    q = 0.0; c = 0.0;
    if (cz > 0.0) { const double a = 1.0 - vb * ds.get(P, d0 + 0), s = fexp(-mj * flog(a, kc), kc); q += pb * cz * (1.0 - a * s) * ds.get(P, d0 + 3); c += cz * s; }
    if (czsw > 0.0) { const double a = 1.0 - vb * ds.get(P, d0 + 1), s = fexp(-mjsw * flog(a, kc), kc); q += pbsw * czsw * (1.0 - a * s) * ds.get(P, d0 + 4); c += czsw * s; }
    if (czswg > 0.0) { const double a = 1.0 - vb * ds.get(P, d0 + 2), s = fexp(-mjswg * flog(a, kc), kc); q += pbswg * czswg * (1.0 - a * s) * ds.get(P, d0 + 5); c += czswg * s; }
  } else {
    const double t0 = cz + czsw + czswg, t1 = cz * mj * ds.get(P, d0 + 0) + czsw * mjsw * ds.get(P, d0 + 1) + czswg * mjswg * ds.get(P, d0 + 2);
    q = vb * (t0 + 0.5 * t1 * vb); c = t0 + t1 * vb;
  }
}
// bias-dependent overlap charge (capMod 2) and capacitance for one side
CH_D void overlap(double vg, double cov, double clW, double ckappa, double ickappa, double& q, double& c) {
  const double t0 = vg + 0.02, t1 = fsqrt(t0 * t0 + 0.08), t2 = 0.5 * (t0 - t1), dt2 = 0.5 * (1.0 - t0 * frcp(t1));
  const double t4 = fsqrt(1.0 - 4.0 * t2 * ickappa);
  q = (cov + clW) * vg - clW * (t2 + 0.5 * ckappa * (t4 - 1.0));
  c = (cov + clW) - clW * (dt2 - dt2 * frcp(t4));
}

// Mode-frame core: currents into the mode drain / source / bulk and the intrinsic charges, as
// dual numbers w.r.t. whatever seeds Vgs, Vds, Vbs carry.
template <int N>
struct B4Core {
  DN<N> iD, iS, iB, qd, qg, qs, qb;
};

// A tap into the core for the noise analysis: values the I-V and the charge half form on their way.  It is compile-time only.
// B4NoTap (the default, every stamp evaluation) has no members and b4_core never names it outside `if constexpr (TAP::on)`;
// B4NoiseTap (b4_noise below) receives the values.
struct B4NoTap { static constexpr bool on = false; };
struct B4NoiseTap {
  static constexpr bool on = true;
  double ids, ueff, vgsteff, abulk, vdseff, rds, esat;   // the I-V half (ids: the channel current of all fingers, mode frame)
  double vgc, t0cv, coxwlcen;                            // the capMod-2 half: Vgsteff,cv, AbulkCV Vdseff,cv, Coxeff Weff,cv NF Leff,cv
  bool has_cv;                                           // false when the card has no intrinsic charge model (capmod 0, xpart < 0)
};

// Vgs, Vds, Vbs come as types of their own: each says which partials it has (b4_device: one each; b4_device_quad: the one
// run-time seeded partial in all three, the dense form).  Straight-line intermediates are `auto` and carry the union of what they
// were made from; where two paths join, the variable is declared with the set of the join (DG, DD, DB, ... below) and both
// sides are widened to it.
template <int N, class K, class DS, class VG, class VD, class VB, class TAP = B4NoTap>
CH_D void b4_core(const K kc, const DS ds, const B4Col P, const VG Vgs, const VD Vds, const VB Vbs, B4Core<N>& o, TAP* tap = nullptr) {
  using namespace k;
  constexpr unsigned MG = VG::mask, MD = VD::mask, MB = VB::mask;
  constexpr bool DENSE = (MG & MD & MB) == (MG | MD | MB);   // constants then carry their zero partials, as in the dense form
  typedef DN<N, dn::from_mask(MG, N)> DG;
  typedef DN<N, dn::from_mask(MD, N)> DD;
  typedef DN<N, dn::from_mask(MB, N)> DB;
  typedef DN<N, dn::from_mask(MG | MD, N)> DGD;
  typedef DN<N, dn::from_mask(MG | MB, N)> DGB;
  typedef DN<N, dn::from_mask(MB | MD, N)> DBD;
  typedef DN<N, dn::from_mask(MG | MD | MB, N)> D;
  auto cst = [](double x) { if constexpr (DENSE) return mkd<N>(x); else return cstd<N>(x); };
  // exp and log below take their coefficients from kc
  auto dexp = [&](const auto a) { return chip::dexp(a, kc); };
  auto dlog = [&](const auto a) { return chip::dlog(a, kc); };
  auto d_sce = [&](const auto a) { return chip::d_sce(a, kc); };
  const double phi = P[B4I_phi], sqrtPhi = P[B4I_sqrtPhi], Vtm = P[B4I_vtm], Leff = P[B4I_leff];
  const double coxe = P[B4I_coxe], itoxe = ds.get(P, B4D_itoxe), icoxe = ds.get(P, B4D_icoxe), iLeff = ds.get(P, B4D_iLeff);

  // ---- effective body bias ----
  DB Vbseff0;
  {
    const double vbsc = P[B4I_vbsc];
    const auto t0 = Vbs - (vbsc + 0.001);
    const auto t1 = dsqrt(t0 * t0 - 0.004 * vbsc);
    if (t0.v >= 0.0) Vbseff0 = 0.5 * (t0 + t1) + vbsc;
    else Vbseff0 = vbsc * (1.0 + (-0.002) / (t1 - t0));
  }
  const double t9b = 0.95 * phi;
  const auto u0b = t9b - Vbseff0 - 0.001;
  const auto Vbseff = t9b - 0.5 * (u0b + dsqrt(u0b * u0b + 0.004 * t9b));
  const auto Phis = phi - Vbseff;
  const auto sqrtPhis = dsqrt(Phis);
  const auto Xdep = sqrtPhis * (P[B4I_Xdep0] * ds.get(P, B4D_isqrtPhi));

  // ---- threshold voltage ----
  const auto sqXdep = dsqrt(Xdep);
  const double f1 = P[B4I_factor1], V0 = P[B4I_vbi_phi];
  auto ltf = [&](double dv2) {
    const auto a = Vbseff * dv2;
    const DB b = (a.v >= -0.5) ? DB(a + 1.0) : DB((1.0 + 3.0 * a) / (3.0 + 8.0 * a));
    return sqXdep * b * f1;
  };
  const auto Theta0 = d_sce(P[B4I_dvt1L] / ltf(P[B4I_dvt2]));
  const auto Delt_vth = Theta0 * (P[B4I_dvt0] * V0);
  const double dvt0w = P[B4I_dvt0w];
  DB T2w = cst(0.0);
  if (dvt0w != 0.0) T2w = d_sce(P[B4I_dvt1wWL] / ltf(P[B4I_dvt2w])) * (dvt0w * V0);
  const auto T1t = P[B4I_lpe0term] + P[B4I_kt1eff] + Vbseff * P[B4I_kt2t];
  DB T3d = P[B4I_eta0] + P[B4I_etab] * Vbseff;
  if (T3d.v < 1.0e-4) T3d = (2.0e-4 - T3d) / (3.0 - 2.0e4 * T3d);
  const auto DIBL_Sft = T3d * Vds * P[B4I_theta0vb0];
  const double vthNW = P[B4I_vthNarrowW], LpeVb = P[B4I_LpeVb], k1ox = P[B4I_k1ox], k2ox = P[B4I_k2ox];
  DBD Vth = P[B4I_vth0t] + (k1ox * sqrtPhis - P[B4I_k1] * sqrtPhi) * LpeVb - k2ox * Vbseff - Delt_vth - T2w +
          (P[B4I_k3] + P[B4I_k3b] * Vbseff) * vthNW + T1t - DIBL_Sft;

  // ---- subthreshold swing ----
  DBD n;
  {
    const auto c1 = EPSSI / Xdep;
    const auto t4 = (P[B4I_nfactor] * c1 + (P[B4I_cdsc] + P[B4I_cdscb] * Vbseff + P[B4I_cdscd] * Vds) * Theta0 + P[B4I_cit]) * icoxe;
    n = (t4.v >= -0.5) ? DBD(t4 + 1.0) : DBD((1.0 + 3.0 * t4) / (3.0 + 8.0 * t4));
  }
  {
    const double dvtp0 = P[B4I_dvtp0];
    if (dvtp0 > 0.0) {
      const auto t0 = -P[B4I_dvtp1] * Vds;
      const DD t2 = (t0.v < -EXP_TH) ? DD(cst(MIN_EXP)) : DD(dexp(t0));
      const auto t3 = Leff + dvtp0 * (1.0 + t2);
      Vth = Vth - n * (Vtm * dlog(Leff / t3));
    }
  }
  // ---- poly depletion ----
  DG Vgs_eff = Vgs;
  {
    const double ngate = P[B4I_ngate], vfbphi = P[B4I_vfb_phi];
    if (ngate > 1.0e18 && ngate < 1.0e25 && Vgs.v > vfbphi) {
      const double iT1p = ds.get(P, B4D_ipolyT1);
      const auto t8 = Vgs - vfbphi;
      const auto t4 = dsqrt(1.0 + t8 * (2.0 * iT1p));
      const auto t2 = 2.0 * t8 / (t4 + 1.0);
      const auto t3 = t2 * t2 * (0.5 * iT1p);
      const auto t7 = 1.07 - t3;
      const auto t6 = dsqrt(t7 * t7 + 0.224);
      Vgs_eff = Vgs - (1.12 - 0.5 * (t7 + t6));
    }
  }
  const auto Vgst = Vgs_eff - Vth;

  // ---- Vgsteff ----
  const auto inVt = recip(n * Vtm);
  D t10, t9;
  {
    const double mstar = P[B4I_mstar], cc = coxe * ds.get(P, B4D_icdep0);
    const auto t1 = mstar * Vgst;
    const auto t2 = t1 * inVt;
    if (t2.v > EXP_TH) t10 = t1;
    else if (t2.v < -EXP_TH) t10 = n * (Vtm * log(1.0 + MIN_EXP));
    else t10 = (n * Vtm) * dlog(1.0 + dexp(t2));
    const auto h2 = (P[B4I_voffcbn] - (1.0 - mstar) * Vgst) * inVt;
    if (h2.v < -EXP_TH) t9 = mstar + n * (cc * MIN_EXP);
    else if (h2.v > EXP_TH) t9 = mstar + n * (cc * MAX_EXP);
    else t9 = mstar + n * (cc * dexp(h2));
  }
  const auto Vgsteff = t10 / t9;

  // ---- Weff, Rds ----
  const auto dsp = sqrtPhis - sqrtPhi;
  D Weff = P[B4I_weff] - 2.0 * (P[B4I_dwg] * Vgsteff + P[B4I_dwb] * dsp);
  if (Weff.v < 2.0e-8) Weff = 2.0e-8 * (4.0e-8 - Weff) / (6.0e-8 - 2.0 * Weff);
  D Rds;
  {
    const auto t2 = recip(1.0 + P[B4I_prwg] * Vgsteff) + P[B4I_prwb] * dsp;
    Rds = P[B4I_rdswmin] + (t2 + dsqrt(t2 * t2 + 0.01)) * P[B4I_rds0h];
  }
  // ---- Abulk ----
  DB Abulk0;
  D Abulk;
  {
    const auto t1 = (0.5 * k1ox * LpeVb) / sqrtPhis + (k2ox - P[B4I_k3b] * vthNW);
    const auto t5 = Leff / (Leff + 2.0 * dsqrt(P[B4I_xj] * Xdep));
    const auto t2 = P[B4I_a0] * t5 + P[B4I_b0term];
    Abulk0 = 1.0 + t1 * t2;
    const auto dAdVg = -t1 * (P[B4I_agsa0] * (t5 * t5 * t5));
    Abulk = Abulk0 + dAdVg * Vgsteff;
    if (Abulk0.v < 0.1) Abulk0 = (0.2 - Abulk0) / (3.0 - 20.0 * Abulk0);
    if (Abulk.v < 0.1) Abulk = (0.2 - Abulk) / (3.0 - 20.0 * Abulk);
    const auto t2k = P[B4I_keta] * Vbseff;
    const DB t0k = (t2k.v >= -0.9) ? DB(recip(1.0 + t2k)) : DB((17.0 + 20.0 * t2k) / (0.8 + t2k));
    Abulk = Abulk * t0k;
    Abulk0 = Abulk0 * t0k;
  }
  // ---- mobility ----
  D iueff;  // 1/ueff
  {
    const int mobmod = (int)P[B4I_mobmod];
    D t5;
    if (mobmod == 0) {
      const auto t3 = (Vgsteff + Vth + Vth) * itoxe;
      t5 = t3 * (P[B4I_ua] + P[B4I_uc] * Vbseff + P[B4I_ub] * t3);
    } else if (mobmod == 1) {
      const auto t3 = (Vgsteff + Vth + Vth) * itoxe;
      t5 = t3 * (P[B4I_ua] + P[B4I_ub] * t3) * (1.0 + P[B4I_uc] * Vbseff);
    } else {
      const auto t0 = (Vgsteff + P[B4I_vtfbphi1]) * itoxe;
      t5 = dexp(P[B4I_eu] * dlog(t0)) * (P[B4I_ua] + P[B4I_uc] * Vbseff);
    }
    const D den = (t5.v >= -0.8) ? D(t5 + 1.0) : D((0.6 + t5) / (7.0 + 10.0 * t5));
    iueff = den * ds.get(P, B4D_iu0temp);
  }
  const auto ueff = recip(iueff);
  // ---- Vdsat ----
  const double vsat = P[B4I_vsattemp];
  const auto WVCoxRds = Weff * Rds * (vsat * coxe);
  const auto Esat = (2.0 * vsat) * iueff;
  const auto EsatL = Esat * Leff;
  const auto iEsatL = recip(EsatL);
  D Lambda;
  {
    const double a1 = P[B4I_a1], a2 = P[B4I_a2];
    if (a1 == 0.0) Lambda = cst(a2);
    else if (a1 > 0.0) {
      const double t0 = 1.0 - a2;
      const auto t1 = t0 - a1 * Vgsteff - 0.0001;
      Lambda = a2 + t0 - 0.5 * (t1 + dsqrt(t1 * t1 + 0.0004 * t0));
    } else {
      const auto t1 = a2 + a1 * Vgsteff - 0.0001;
      Lambda = 0.5 * (t1 + dsqrt(t1 * t1 + 0.0004 * a2));
    }
  }
  const auto iLam = recip(Lambda);
  const auto Vgst2Vtm = Vgsteff + 2.0 * Vtm;
  const auto iVgst2Vtm = recip(Vgst2Vtm);
  D Vdsat;
  if (Rds.v == 0.0 && Lambda.v == 1.0) Vdsat = EsatL * Vgst2Vtm / (Abulk * EsatL + Vgst2Vtm);
  else {
    const auto t9 = Abulk * WVCoxRds;
    const auto t0 = 2.0 * Abulk * (t9 - 1.0 + iLam);
    const auto t1 = Vgst2Vtm * (2.0 * iLam - 1.0) + Abulk * EsatL + 3.0 * (Vgst2Vtm * t9);
    const auto t2 = Vgst2Vtm * (EsatL + 2.0 * (Vgst2Vtm * WVCoxRds));
    Vdsat = (t1 - dsqrt(t1 * t1 - 2.0 * t0 * t2)) / t0;
  }
  // ---- Vdseff ----
  D Vdseff;
  {
    const double delta = P[B4I_delta];
    const auto t1 = Vdsat - Vds - delta;
    const auto t2 = dsqrt(t1 * t1 + 4.0 * delta * Vdsat);
    if (t1.v >= 0.0) Vdseff = Vdsat - 0.5 * (t1 + t2);
    else Vdseff = Vdsat * (1.0 - (2.0 * delta) / (t2 - t1));
    if (Vds.v == 0.0) Vdseff = Vds;
    if (Vdseff.v > Vds.v) Vdseff = Vds;
  }
  const auto diffVds = Vds - Vdseff;
  // ---- Vasat ----
  const auto Vasat = (EsatL + Vdsat + 2.0 * (WVCoxRds * Vgsteff) * (1.0 - 0.5 * Abulk * Vdsat * iVgst2Vtm)) / ((2.0 * iLam - 1.0) + WVCoxRds * Abulk);
  // ---- channel conductance ----
  D Idl;
  {
    const auto t0 = (Vgsteff + P[B4I_vtfbphi2]) * (0.5 * ds.get(P, B4D_itoxp8));
    const auto Tcen = 1.9e-9 / (1.0 + dexp(0.7 * dlog(t0)));
    const double coxp = P[B4I_coxp];
    const auto Coxeff = (EPSSI * coxp) / (EPSSI + coxp * Tcen);
    const auto beta = ueff * Coxeff * Weff * iLeff;
    const auto fg1 = Vgsteff * (1.0 - 0.5 * Vdseff * Abulk * iVgst2Vtm);
    const auto gche = beta * fg1 / (1.0 + Vdseff * iEsatL);
    Idl = gche / (1.0 + gche * Rds);
  }
  // ---- output resistance ----
  const double fpL = P[B4I_fproutL];
  const D FP = (fpL <= 0.0) ? D(cst(1.0)) : D(recip(1.0 + fpL * iVgst2Vtm));
  D Pvag;
  {
    const auto t9 = (P[B4I_pvag] * iEsatL) * Vgsteff;
    Pvag = (t9.v > -0.9) ? D(t9 + 1.0) : D((0.8 + t9) / (17.0 + 20.0 * t9));
  }
  D iCclm, VACLM;  // 1/Cclm
  {
    const double pl = P[B4I_pclmlitl];
    if (pl > 0.0 && diffVds.v > 1.0e-10) {
      const auto Cclm = FP * Pvag * (1.0 + Rds * Idl) * (Leff + Vdsat * ueff * (0.5 * ds.get(P, B4D_ivsat))) * ds.get(P, B4D_ipclmlitl);
      iCclm = recip(Cclm);
      VACLM = Cclm * diffVds;
    } else { iCclm = cst(1.0 / MAX_EXP); VACLM = cst(MAX_EXP); }
  }
  D iVADIBL;
  {
    const double th = P[B4I_thetaRout];
    if (th > MIN_EXP) {
      const auto t8 = Abulk * Vdsat;
      const auto va0 = (Vgst2Vtm - Vgst2Vtm * t8 / (Vgst2Vtm + t8)) * ds.get(P, B4D_ithetaRout);
      const auto t7 = P[B4I_pdiblb] * Vbseff;
      const DB f7 = (t7.v >= -0.9) ? DB(recip(1.0 + t7)) : DB((17.0 + 20.0 * t7) / (0.8 + t7));
      const auto va = va0 * f7;
      iVADIBL = recip(va * Pvag);
    } else iVADIBL = cst(1.0 / MAX_EXP);
  }
  D iVADITS;
  {
    const double pdits = P[B4I_pdits];
    if (pdits > MIN_EXP) {
      const auto t0 = P[B4I_pditsd] * Vds;
      const DD t1 = (t0.v > EXP_TH) ? DD(cst(MAX_EXP)) : DD(dexp(t0));
      iVADITS = recip((1.0 + P[B4I_pditslL] * t1) * ds.get(P, B4D_ipdits) * FP);
    } else iVADITS = cst(1.0 / MAX_EXP);
  }
  D iVASCBE;
  {
    const double ps2 = P[B4I_pscbe2], ps1l = P[B4I_pscbe1l];
    if (ps2 > 0.0) {
      if (diffVds.v > ps1l / EXP_TH) iVASCBE = (ps2 * iLeff) * dexp(-ps1l / diffVds);
      else iVASCBE = cst(ps2 * iLeff / MAX_EXP);
    } else iVASCBE = cst(1.0 / MAX_EXP);
  }
  D Idsa = Idl * (1.0 + diffVds * iVADIBL);
  Idsa = Idsa * (1.0 + diffVds * iVADITS);
  Idsa = Idsa * (1.0 + dlog((Vasat + VACLM) / Vasat) * iCclm);
  D Isub = cst(0.0);
  {
    const double aL = P[B4I_alphaL], beta0 = P[B4I_beta0];
    if (aL > 0.0 && beta0 > 0.0) {
      D t1;
      if (diffVds.v > beta0 / EXP_TH) t1 = aL * diffVds * dexp(-beta0 / diffVds);
      else t1 = (aL * MIN_EXP) * diffVds;
      Isub = t1 * (Idsa * Vdseff);
    }
  }
  const double nf = P[B4I_nf];
  const auto Ids = Idsa * (1.0 + diffVds * iVASCBE) * Vdseff * nf;
  Isub = Isub * nf;
  if constexpr (TAP::on) {
    tap->ids = Ids.v; tap->ueff = ueff.v; tap->vgsteff = Vgsteff.v; tap->abulk = Abulk.v; tap->vdseff = Vdseff.v; tap->rds = Rds.v; tap->esat = Esat.v;
    tap->vgc = 0.0; tap->t0cv = 0.0; tap->coxwlcen = 0.0; tap->has_cv = false;
  }
  // ---- GIDL / GISL ----
  D Igidl = cst(0.0), Igisl = cst(0.0);
  {
    const double agW = P[B4I_agidlW];
    if (agW > 0.0) {
      const double bg = P[B4I_bgidl], cg = P[B4I_cgidl], eg = P[B4I_egidl], it3x = ds.get(P, B4D_itoxe3);
      const auto Vbd = Vbs - Vds;
      const auto t1 = (Vds - Vgs_eff - eg) * it3x;
      if (t1.v > 0.0 && Vbd.v <= 0.0) {
        const auto t2 = bg / t1;
        const DGD ig = (t2.v < 100.0) ? DGD(agW * t1 * dexp(-t2)) : DGD((agW * 3.720075976e-44) * t1);
        const auto t5 = -Vbd * Vbd * Vbd;
        Igidl = ig * (t5 / (cg + t5));
      }
      const auto s1 = (-Vgs_eff - eg) * it3x;
      if (s1.v > 0.0 && Vbs.v <= 0.0) {
        const auto t2 = bg / s1;
        const DG ig = (t2.v < 100.0) ? DG(agW * s1 * dexp(-t2)) : DG((agW * 3.720075976e-44) * s1);
        const auto t5 = -Vbs * Vbs * Vbs;
        Igisl = ig * (t5 / (cg + t5));
      }
    }
  }
  // ---- intrinsic charges (capMod 2) ----
  D qg = cst(0.0), qb = cst(0.0), qsm = cst(0.0), qdm = cst(0.0);
  const double xpart = P[B4I_xpart];
  if (xpart >= 0.0 && (int)P[B4I_capmod] != 0) {
    const DB VbseffCV = (Vbseff.v < 0.0) ? DB(Vbseff) : DB(phi - Phis);
    const double CoxWL = P[B4I_CoxWL], vfbzb = P[B4I_vfbzb], Cox = P[B4I_coxp], Tox = P[B4I_toxp8], ldeb = P[B4I_ldeb];
    const double iTox = ds.get(P, B4D_itoxp8), cwl = CoxWL * icoxe;
    const auto T0q = n * (Vtm * P[B4I_noff]);
    const auto T1q = (Vgst - P[B4I_voffcv]) / T0q;
    D Vgc;
    if (T1q.v > EXP_TH) Vgc = Vgst - P[B4I_voffcv];
    else if (T1q.v < -EXP_TH) Vgc = T0q * log(1.0 + MIN_EXP);
    else Vgc = T0q * dlog(1.0 + dexp(T1q));
    const auto V3 = vfbzb - Vgs_eff + VbseffCV - 0.02;
    const auto Vfbeff = vfbzb - 0.5 * (V3 + dsqrt(V3 * V3 + ((vfbzb <= 0.0) ? -0.08 * vfbzb : 0.08 * vfbzb)));
    const auto tm = (Vgs_eff - VbseffCV - vfbzb) * (P[B4I_acde] * iTox);
    DGB Tcen0;
    if (tm.v > -EXP_TH && tm.v < EXP_TH) Tcen0 = ldeb * dexp(tm);
    else Tcen0 = cst(tm.v <= -EXP_TH ? ldeb * MIN_EXP : ldeb * MAX_EXP);
    const double LINK = 1.0e-11 * Tox;  // 1e-3 * toxp
    const auto V3c = ldeb - Tcen0 - LINK;
    const auto Tcen1 = ldeb - 0.5 * (V3c + dsqrt(V3c * V3c + 4.0 * LINK * ldeb));
    // Coxeff = Cox*Ccen/(Cox+Ccen) with Ccen = EPSSI/Tcen  =  Cox*EPSSI/(Cox*Tcen + EPSSI)
    const auto CoxWLcen1 = (Cox * EPSSI * cwl) / (Cox * Tcen1 + EPSSI);
    const auto Qac0 = CoxWLcen1 * (Vfbeff - vfbzb);
    const double h0 = 0.5 * k1ox;
    const auto T3s = Vgs_eff - Vfbeff - VbseffCV - Vgc;
    D T1s;
    if (k1ox == 0.0) T1s = cst(0.0);
    else if (T3s.v < 0.0) T1s = h0 + T3s * ds.get(P, B4D_ik1ox);
    else T1s = dsqrt(h0 * h0 + T3s);
    const auto Qsub0 = CoxWLcen1 * (k1ox * (T1s - h0));
    const double T0d = (k1ox <= 0.0) ? 0.5 * sqrtPhi : k1ox * sqrtPhi;   // Den (b4_derive): 0.25 moinVtm, or moinVtm k1ox^2
    const auto DeltaPhi = Vtm * dlog(1.0 + (2.0 * T0d + Vgc) * Vgc * ds.get(P, B4D_iDen));
    const auto T3t = 4.0 * (Vth - vfbzb - phi);
    const auto T0t = ((T3t.v >= 0.0) ? D(Vgc + T3t) : D(Vgc + 1.0e-20)) * (0.5 * iTox);
    const auto Tcen = 1.9e-9 / (1.0 + dexp(0.7 * dlog(T0t)));
    const auto CoxWLcen = (Cox * EPSSI * cwl) / (Cox * Tcen + EPSSI);
    const auto AbulkCV = Abulk0 * P[B4I_abulkCVfactor];
    const auto T1 = Vgc - DeltaPhi;
    const auto VdsatCV = T1 / AbulkCV;
    const auto T0v = VdsatCV - Vds - 0.02;
    const auto T1v = dsqrt(T0v * T0v + 0.08 * VdsatCV);
    D VdseffCV;
    if (T0v.v >= 0.0) VdseffCV = VdsatCV - 0.5 * (T0v + T1v);
    else VdseffCV = VdsatCV * (1.0 - 0.04 / (T1v - T0v));
    if (Vds.v == 0.0) VdseffCV = Vds;
    const auto T0 = AbulkCV * VdseffCV;
    const auto T2 = 12.0 * (T1 - 0.5 * T0 + 1.0e-20);
    const auto iT2 = recip(T2);
    const auto T3 = T0 * iT2;
    if constexpr (TAP::on) { tap->vgc = Vgc.v; tap->t0cv = T0.v; tap->coxwlcen = CoxWLcen.v; tap->has_cv = true; }
    qg = CoxWLcen * (T1 - T0 * (0.5 - T3));
    qb = CoxWLcen * (1.0 - AbulkCV) * (0.5 * VdseffCV - T3 * VdseffCV);
    if (xpart > 0.5) qsm = -CoxWLcen * (0.5 * T1 + 0.25 * T0 - 0.5 * T0 * T3);
    else if (xpart < 0.5) {
      const auto T4b = T1 * ((2.0 / 3.0) * T0 * T0 + T1 * (T1 - (4.0 / 3.0) * T0)) - (2.0 / 15.0) * T0 * T0 * T0;
      qsm = -(72.0 * CoxWLcen * (iT2 * iT2)) * T4b;  // 0.5/(T2/12)^2 = 72/T2^2
    } else qsm = -0.5 * qg;
    qg = qg + Qac0 + Qsub0 - qb;
    qb = qb - (Qac0 + Qsub0);
    qdm = -(qg + qb + qsm);
  }
  // currents into the device: D': Ids + Isub + Igidl ; S': -Ids + Igisl ; B: -Isub - Igidl - Igisl
  o.iD = Ids + Isub + Igidl; o.iS = Igisl - Ids; o.iB = -(Isub + Igidl + Igisl);
  o.qd = qdm; o.qg = qg; o.qs = qsm; o.qb = qb;
}

// Junction diodes, junction charges and overlap charges on the TRUE terminals (type-normalised
// voltages): 5 two-terminal elements (a, b, value x, derivative dx w.r.t. v_a - v_b).
struct B4Two {
  double ibs, gbs, ibd, gbd, qbs, cbs, qbd, cbd, qgd, cgd, qgs, cgs, qgb, cgb;
};
template <class K, class DS>
CH_D void b4_two_terminal(const K kc, const DS ds, const B4Col P, double vgs, double vds, double vbs, double gmin, B4Two& t) {
  const double vbd = vbs - vds;
  diode(kc, ds, P, B4D_iNvtms, vbs, P[B4I_Isbs], P[B4I_vjsmFwd], P[B4I_IVjsmFwd], gmin, t.ibs, t.gbs);
  diode(kc, ds, P, B4D_iNvtmd, vbd, P[B4I_Isbd], P[B4I_vjdmFwd], P[B4I_IVjdmFwd], gmin, t.ibd, t.gbd);
  junction(kc, ds, P, B4D_iPhiBS, vbs, P[B4I_czbs], P[B4I_czbssw], P[B4I_czbsswg], P[B4I_PhiBS], P[B4I_PhiBSWS], P[B4I_PhiBSWGS], P[B4I_mjs], P[B4I_mjsws], P[B4I_mjswgs], t.qbs, t.cbs);
  junction(kc, ds, P, B4D_iPhiBD, vbd, P[B4I_czbd], P[B4I_czbdsw], P[B4I_czbdswg], P[B4I_PhiBD], P[B4I_PhiBSWD], P[B4I_PhiBSWGD], P[B4I_mjd], P[B4I_mjswd], P[B4I_mjswgd], t.qbd, t.cbd);
  if ((int)P[B4I_capmod] != 0) {
    overlap(vgs - vds, P[B4I_cgdo], P[B4I_cgdlW], P[B4I_ckappad], ds.get(P, B4D_ickappad), t.qgd, t.cgd);
    overlap(vgs, P[B4I_cgso], P[B4I_cgslW], P[B4I_ckappas], ds.get(P, B4D_ickappas), t.qgs, t.cgs);
    t.cgb = P[B4I_cgbo]; t.qgb = t.cgb * (vgs - vbs);
  } else { t.qgd = t.cgd = t.qgs = t.cgs = t.qgb = t.cgb = 0.0; }
}

// One lane per instance.  out[40] = {I[4], Q[4], G[16], C[16]} for terminals (d,g,s,b);
// the multiplier is applied by the caller.
template <class K = KLit, class DS = B4DHere>
CH_D void b4_device(const B4Col P, double vd, double vg, double vs, double vb, double gmin, double* out, const K kc = K{}, const DS ds = DS{}) {
  const double tp = P[B4I_type];
  const double vds = tp * (vd - vs), vgs = tp * (vg - vs), vbs = tp * (vb - vs);
  const bool fwd = vds >= 0.0;
  // one partial each: everything in front of Vgst depends on one or two of the three
  const auto Vgs = seed<3, 0>(fwd ? vgs : vgs - vds);
  const auto Vds = seed<3, 1>(fwd ? vds : -vds);
  const auto Vbs = seed<3, 2>(fwd ? vbs : vbs - vds);
  B4Core<3> c;
  b4_core<3>(kc, ds, P, Vgs, Vds, Vbs, c);
  double* I = out; double* Qo = out + 4; double* G = out + 8; double* C = out + 24;
  // mode-frame stamp, rows/cols (D', G, S', B); d/dS' = -(sum of the three partials)
  // (a partial that x does not have reads as its zero: +0.0, or -0.0 where the dense form's literal zero was negated on the way
  // (state ZN) — the value is the same, and so is the sign the dense form stores)
  auto put = [&](int row, const auto& x, double* val, double* M) {
    val[row] = x.v; M[row * 4 + 0] = x.get(1); M[row * 4 + 1] = x.get(0); M[row * 4 + 3] = x.get(2); M[row * 4 + 2] = -(x.get(0) + x.get(1) + x.get(2));
  };
  put(0, c.iD, I, G); put(1, cstd<3>(0.0), I, G); put(2, c.iS, I, G); put(3, c.iB, I, G);
  put(0, c.qd, Qo, C); put(1, c.qg, Qo, C); put(2, c.qs, Qo, C); put(3, c.qb, Qo, C);
  // map mode frame -> true (d,g,s,b): exchange index 0 and 2 (rows and columns) when reversed.
  // Static indices under one runtime predicate keep everything in registers (no scratch).
  if (!fwd) {
    auto sw = [](double& x, double& y) { const double t = x; x = y; y = t; };
    sw(I[0], I[2]); sw(Qo[0], Qo[2]);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) { sw(G[0 * 4 + cc], G[2 * 4 + cc]); sw(C[0 * 4 + cc], C[2 * 4 + cc]); }
#pragma unroll
    for (int r = 0; r < 4; ++r) { sw(G[r * 4 + 0], G[r * 4 + 2]); sw(C[r * 4 + 0], C[r * 4 + 2]); }
  }
  B4Two t;
  b4_two_terminal(kc, ds, P, vgs, vds, vbs, gmin, t);
  auto two = [&](double* val, double* M, int a, int b, double x, double dx) {
    val[a] += x; val[b] -= x;
    M[a * 4 + a] += dx; M[a * 4 + b] -= dx; M[b * 4 + a] -= dx; M[b * 4 + b] += dx;
  };
  two(I, G, 3, 2, t.ibs, t.gbs); two(I, G, 3, 0, t.ibd, t.gbd);
  two(Qo, C, 3, 2, t.qbs, t.cbs); two(Qo, C, 3, 0, t.qbd, t.cbd);
  two(Qo, C, 1, 0, t.qgd, t.cgd); two(Qo, C, 1, 2, t.qgs, t.cgs); two(Qo, C, 1, 3, t.qgb, t.cgb);
#pragma unroll
  for (int r = 0; r < 4; ++r) { I[r] *= tp; Qo[r] *= tp; }
}

// Four lanes per instance (a quad, lanes 4q..4q+3 of one wavefront).  Lane `sub` seeds ONE partial
// (0: Vgs', 1: Vds', 2: Vbs', 3: none), so the dual-number arithmetic per lane shrinks from
// 1+3 to 1+1 components; the S' column is the negated sum of the other three, formed with two
// quad shuffles.  Each lane then owns ONE column of the 4x4 G and C stamps and writes it straight
// into the 40-slot staging record `st` (scaled by the multiplier m); lane 3 also writes I and Q.
CH_D void b4_device_quad(const B4Col P, double vd, double vg, double vs, double vb, double gmin, int sub, double m, double* st) {
  const double tp = P[B4I_type];
  const double vds = tp * (vd - vs), vgs = tp * (vg - vs), vbs = tp * (vb - vs);
  const bool fwd = vds >= 0.0;
  typedef DN<1> D1;
  D1 Vgs = mkd<1>(fwd ? vgs : vgs - vds), Vds = mkd<1>(fwd ? vds : -vds), Vbs = mkd<1>(fwd ? vbs : vbs - vds);
  Vgs.p[0] = sub == 0 ? 1.0 : 0.0; Vds.p[0] = sub == 1 ? 1.0 : 0.0; Vbs.p[0] = sub == 2 ? 1.0 : 0.0;
  B4Core<1> c;
  b4_core<1>(KLit{}, B4DHere{}, P, Vgs, Vds, Vbs, c);
  // this lane's column in the mode frame (D'=0, G=1, S'=2, B=3): sub 0 -> G, 1 -> D', 2 -> B, 3 -> S'
  auto quad_sum = [](double x) { x += __shfl_xor(x, 1); x += __shfl_xor(x, 2); return x; };
  auto colval = [&](const D1& x) { const double sum = quad_sum(x.p[0]); return sub == 3 ? -sum : x.p[0]; };
  // mode-frame rows D', G, S', B
  double gI[4] = {colval(c.iD), 0.0, colval(c.iS), colval(c.iB)};
  double gQ[4] = {colval(c.qd), colval(c.qg), colval(c.qs), colval(c.qb)};
  double I4[4] = {c.iD.v, 0.0, c.iS.v, c.iB.v}, Q4[4] = {c.qd.v, c.qg.v, c.qs.v, c.qb.v};
  int col = sub == 0 ? 1 : (sub == 1 ? 0 : (sub == 2 ? 3 : 2));
  if (!fwd) {  // mode frame -> true frame: exchange D' and S' (rows, and this lane's column label)
    auto sw = [](double& x, double& y) { const double t = x; x = y; y = t; };
    sw(gI[0], gI[2]); sw(gQ[0], gQ[2]); sw(I4[0], I4[2]); sw(Q4[0], Q4[2]);
    col = col == 0 ? 2 : (col == 2 ? 0 : col);
  }
  B4Two t;
  b4_two_terminal(KLit{}, B4DHere{}, P, vgs, vds, vbs, gmin, t);
  // two-terminal element between rows (a,b): this lane's column gets +dx on row a / -dx on row b if
  // col == a, the opposite if col == b
  auto two = [&](double* val, double* gcol, int a, int b, double x, double dx) {
    val[a] += x; val[b] -= x;
    const double s = col == a ? dx : (col == b ? -dx : 0.0);
    gcol[a] += s; gcol[b] -= s;
  };
  two(I4, gI, 3, 2, t.ibs, t.gbs); two(I4, gI, 3, 0, t.ibd, t.gbd);
  two(Q4, gQ, 3, 2, t.qbs, t.cbs); two(Q4, gQ, 3, 0, t.qbd, t.cbd);
  two(Q4, gQ, 1, 0, t.qgd, t.cgd); two(Q4, gQ, 1, 2, t.qgs, t.cgs); two(Q4, gQ, 1, 3, t.qgb, t.cgb);
#pragma unroll
  for (int r = 0; r < 4; ++r) { st[8 + r * 4 + col] = m * gI[r]; st[24 + r * 4 + col] = m * gQ[r]; }
  if (sub == 3) {
    const double mt = m * tp;
#pragma unroll
    for (int r = 0; r < 4; ++r) { st[r] = mt * I4[r]; st[4 + r] = mt * Q4[r]; }
  }
}

// Noise evaluation of one instance at true terminal voltages: one run of the core with the noise tap, in the mode frame the stamp
// evaluation takes (a device whose drain and source are exchanged gives the operand row of the forward one), partials dropped.
// op[B4NO_COUNT] is the operand row b4_noise_records (ch_b4_noise.hpp) reads.  ids, weff nf and qinv are those of all NF fingers, so
// rds is the Rds the current half forms (one finger's) over NF: the series resistance of the whole device.  Returns false when the card has no intrinsic charge
// model to take qinv from.
CH_D bool b4_noise(const B4Col P, double vd, double vg, double vs, double vb, double* op) {
  const double tp = P[B4I_type];
  const double vds = tp * (vd - vs), vgs = tp * (vg - vs), vbs = tp * (vb - vs);
  const bool fwd = vds >= 0.0;
  const auto Vgs = seed<3, 0>(fwd ? vgs : vgs - vds);
  const auto Vds = seed<3, 1>(fwd ? vds : -vds);
  const auto Vbs = seed<3, 2>(fwd ? vbs : vbs - vds);
  B4Core<3> c;
  B4NoiseTap t;
  b4_core<3>(KLit{}, B4DHere{}, P, Vgs, Vds, Vbs, c, &t);
  op[B4NO_ids] = t.ids; op[B4NO_ueff] = t.ueff; op[B4NO_vgsteff] = t.vgsteff; op[B4NO_abulk] = t.abulk; op[B4NO_vdseff] = t.vdseff;
  op[B4NO_vds] = Vds.v; op[B4NO_rds] = t.rds / P[B4I_nf]; op[B4NO_esat] = t.esat; op[B4NO_litl] = P[B4I_litl]; op[B4NO_leff] = P[B4I_leff];
  op[B4NO_weffnf] = P[B4I_weff] * P[B4I_nf]; op[B4NO_coxe] = P[B4I_coxe]; op[B4NO_cdep0] = P[B4I_cdep0]; op[B4NO_cit] = P[B4I_cit]; op[B4NO_vtm] = P[B4I_vtm];
  // qinv = Coxeff Weff,cv NF Leff,cv [Vgsteff,cv - T0/2 + T0^2 / (12 (Vgsteff,cv - T0/2 + 1e-20))],  T0 = AbulkCV Vdseff,cv
  const double h = t.vgc - 0.5 * t.t0cv;
  op[B4NO_qinv] = t.coxwlcen * (h + t.t0cv * t.t0cv / (12.0 * (h + 1.0e-20)));
  return t.has_cv;
}
#endif  // __HIPCC__

}  // namespace chip
