// Host test of the gather schedule built with padded strides (cedarsim.jl_amd/csrc/ch_gather_plan.hpp, GatherStrides), under ASan /
// UBSan (tests/test_host_gather_strides.py).  For every class and both register-LU sizes that take it: the padded plan has the
// unpadded plan's records (lanes, trips, sources, counts, flags) and differs in the destination offsets alone; every destination
// lies inside its image and decodes to the (row, column) or vector entry the unpadded plan's offset decodes to; the entries the
// kernel reaches as Cm[oc - nc] (F) and Cm[oc + nc] (hq) are the vectors behind C's nc rows; no pad entry is ever a destination; and a
// replay of the kernel's trip loop into images that hold the pad pattern (identity rows, +0.0 / -0.0 pad columns) leaves that
// pattern as it is and every real entry with the bits of the unpadded replay.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ch_gather_plan.hpp"

using namespace chip;

static int n_bad = 0, n_plans = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++n_bad; std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

constexpr int CO = 16, QO = 4;   // StampLayout<false>: charge-Jacobian and charge offsets of a stamp record

struct Class {
  int nc = 0;
  std::vector<int> mat_ptr, vec_ptr;
  std::vector<uint16_t> src16;
  int n_mat_src = 0;
};
static Class make_class(int nc, int dens, int heavy, std::mt19937& rng) {
  Class c; c.nc = nc;
  std::uniform_int_distribution<int> off(0, 1500);
  c.mat_ptr.push_back(0);
  for (int e = 0; e < nc * nc; ++e) {
    int cnt = 0;
    if ((int)(rng() % 10) < dens) cnt = (rng() % 8 == 0) ? 1 + (int)(rng() % heavy) : 1 + (int)(rng() % 3);
    for (int k = 0; k < cnt; ++k) c.src16.push_back((uint16_t)off(rng));
    c.mat_ptr.push_back((int)c.src16.size());
  }
  c.n_mat_src = (int)c.src16.size();
  c.vec_ptr.push_back(0);
  for (int i = 0; i < nc; ++i) { const int cnt = (int)(rng() % (heavy + 1)); for (int k = 0; k < cnt; ++k) c.src16.push_back((uint16_t)off(rng)); c.vec_ptr.push_back((int)c.src16.size() - c.n_mat_src); }
  return c;
}

// the wave region from A on, as tran_persistent_kernel lays it out: A[rows_a * lda] | Cm[nc * ldc] | xl xp Fv Qv hq [5 * nc]
struct Region {
  int nc, lda, ldc, rows_a;
  std::vector<double> d;
  size_t nA() const { return (size_t)rows_a * lda; }
  size_t nC() const { return (size_t)nc * ldc; }
  double* A() { return d.data(); }
  double* Cm() { return d.data() + nA(); }
};
constexpr double SENT = 12345.678;
static Region make_region(int nc, GatherStrides gs, const std::vector<double>& hq) {
  Region r; r.nc = nc; r.lda = gs.lda; r.ldc = gs.ldc; r.rows_a = gs.padded(nc) ? gs.lda - 1 : nc;
  r.d.assign(r.nA() + r.nC() + 5 * (size_t)nc, SENT);
  // what the kernel writes once per transient: zeros (the gather rewrites the structural non-zeros only), and the pad pattern
  for (size_t i = 0; i < r.nA() + r.nC(); ++i) r.d[i] = 0.0;
  if (gs.padded(nc)) {
    for (int i = 0; i < r.rows_a; ++i) for (int j = 0; j < r.lda; ++j) r.A()[i * r.lda + j] = (i >= nc && j == i) ? 1.0 : 0.0;
    for (int i = 0; i < nc; ++i) for (int j = 0; j < r.ldc; ++j) r.Cm()[i * r.ldc + j] = j >= nc ? -0.0 : 0.0;
  }
  for (int i = 0; i < nc; ++i) r.Cm()[r.nC() + 4 * nc + i] = hq[i];
  return r;
}
// the kernel's trip loop (ch_persist.hpp), lane by lane
static void replay(const GatherPlan& gp, Region& r, const std::vector<double>& st, double alpha0) {
  const int* head = gp.words.data(); const int* srcw = head + GP_HEAD_INTS; const int* ctlw = srcw + 2 * (size_t)gp.R;
  double* A = r.A(); double* Cm = r.Cm(); const int nc = r.nc;
  double s1[64], s2[64];
  for (int l = 0; l < 64; ++l) s1[l] = s2[l] = 0.0;
  for (int tr = 0; tr < gp.T; ++tr) for (int l = 0; l < 64; ++l) {
    const int b = (int)((uint32_t)head[l] & 0xffffu), n_l = (int)((uint32_t)head[l] >> 16), rec = tr < n_l ? b + tr : 0;
    const uint32_t ox = (uint32_t)srcw[2 * rec], oy = (uint32_t)srcw[2 * rec + 1]; const unsigned cw = (unsigned)ctlw[rec];
    const int n = (int)(cw & GP_N_MASK);
    const bool vec = cw & GP_VEC;
    const int off2 = vec ? QO : CO;
    const int o[4] = {(int)(ox & 0xffffu), (int)(ox >> 16), (int)(oy & 0xffffu), (int)(oy >> 16)};
    const int oa = (int)((cw >> GP_A_SHIFT) & GP_OFS_MASK), oc = (int)(cw >> GP_C_SHIFT);
    const double hqe = Cm[oc + nc];   // (every lane reads it, as in the kernel: must lie inside the region for the idle record too)
    for (int k = 0; k < n; ++k) { s1[l] += st[o[k]]; s2[l] += st[o[k] + off2]; }
    if (cw & GP_END) {
      const double G = s1[l] + alpha0 * s2[l];
      if (vec) { const double F = G + hqe; Cm[oc - nc] = F; A[oa] = -F; }
      else A[oa] = G;
      Cm[oc] = s2[l];
      s1[l] = 0.0; s2[l] = 0.0;
    }
  }
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static void check_pair(const Class& c, int NC, const char* name, std::mt19937& rng) {
  ++n_plans;
  const int nc = c.nc;
  const GatherStrides gu = GatherStrides::unpadded(nc), gs{NC + 1, NC};
  GatherPlan pu, pp;
  const bool bu = pu.build(nc, c.mat_ptr, c.vec_ptr, c.src16, c.n_mat_src), bp = pp.build(nc, c.mat_ptr, c.vec_ptr, c.src16, c.n_mat_src, gs);
  CHECK(bu && bp, "%s: nc %d NC %d build %d %d", name, nc, NC, (int)bu, (int)bp);
  if (!bu || !bp) return;
  CHECK(gs.padded(nc) == (nc < NC) && !gu.padded(nc), "%s: padded()", name);
  CHECK(gs.extra_doubles(nc) == NC * (NC + 1) + nc * NC - nc * (nc + 1) - nc * nc && gu.extra_doubles(nc) == 0, "%s: extra doubles %d", name, gs.extra_doubles(nc));
  CHECK(pu.T == pp.T && pu.R == pp.R && pu.words.size() == pp.words.size(), "%s: T %d %d R %d %d", name, pu.T, pp.T, pu.R, pp.R);
  if (pu.words.size() != pp.words.size()) return;
  const size_t ctl0 = (size_t)GP_HEAD_INTS + 2 * (size_t)pu.R;
  for (size_t i = 0; i < ctl0; ++i) CHECK(pu.words[i] == pp.words[i], "%s: head / source word %zu differs", name, i);
  const unsigned low = (1u << GP_A_SHIFT) - 1u;
  std::vector<char> hitA((size_t)NC * (NC + 1), 0), hitC((size_t)nc * NC + 5 * (size_t)nc, 0);
  for (int rec = 0; rec < pu.R; ++rec) {
    const unsigned cu = (unsigned)pu.words[ctl0 + rec], cp = (unsigned)pp.words[ctl0 + rec];
    CHECK((cu & low) == (cp & low), "%s: record %d count / flags differ", name, rec);
    if (!(cp & GP_END)) { CHECK(cu == cp && (cp >> GP_A_SHIFT) == 0, "%s: record %d carries offsets without closing an item", name, rec); continue; }
    const bool vec = cp & GP_VEC;
    const int oau = (int)((cu >> GP_A_SHIFT) & GP_OFS_MASK), ocu = (int)(cu >> GP_C_SHIFT), oap = (int)((cp >> GP_A_SHIFT) & GP_OFS_MASK), ocp = (int)(cp >> GP_C_SHIFT);
    if (vec) {
      const int eu = ocu - (nc * nc + 3 * nc), ep = ocp - (nc * NC + 3 * nc);
      CHECK(eu >= 0 && eu < nc && ep == eu, "%s: record %d row of F / Q %d vs %d", name, rec, ep, eu);
      CHECK(oau == eu * (nc + 1) + nc && oap == ep * (NC + 1) + NC, "%s: record %d right-hand side offsets %d %d", name, rec, oau, oap);
      // Fv[e] and hq[e] as the kernel reaches them: one row of nc below and above Qv[e], behind C's nc rows of NC
      CHECK(ocp - nc == nc * NC + 2 * nc + ep && ocp + nc == nc * NC + 4 * nc + ep, "%s: record %d F / hq relation", name, rec);
      if (ep >= 0 && ep < nc) { ++hitA[(size_t)oap]; ++hitC[(size_t)ocp]; ++hitC[(size_t)(ocp - nc)]; }
    } else {
      const int ru = ocu / nc, colu = ocu % nc, rp = ocp / NC, colp = ocp % NC;
      CHECK(ocu < nc * nc && rp == ru && colp == colu && rp < nc && colp < nc, "%s: record %d C entry (%d, %d) vs (%d, %d)", name, rec, rp, colp, ru, colu);
      CHECK(oau == ru * (nc + 1) + colu && oap == rp * (NC + 1) + colp, "%s: record %d A entry offsets %d %d", name, rec, oau, oap);
      if (rp < nc && colp < nc) { ++hitA[(size_t)oap]; ++hitC[(size_t)ocp]; }
    }
  }
  for (int i = 0; i < NC; ++i) for (int j = 0; j <= NC; ++j) {
    const bool pad = i >= nc || (j >= nc && j < NC);
    if (pad) CHECK(hitA[(size_t)i * (NC + 1) + j] == 0, "%s: pad entry (%d, %d) of A is a destination", name, i, j);
    else CHECK(hitA[(size_t)i * (NC + 1) + j] <= 1, "%s: entry (%d, %d) of A is a destination twice", name, i, j);
  }
  for (int i = 0; i < nc; ++i) for (int j = nc; j < NC; ++j) CHECK(hitC[(size_t)i * NC + j] == 0, "%s: pad entry (%d, %d) of C is a destination", name, i, j);
  // ---- replay into both layouts ----
  std::uniform_real_distribution<double> val(-1.0, 1.0);
  std::vector<double> st(1500 + CO + 1), hq(nc);
  for (double& v : st) { v = std::ldexp(val(rng), (int)(rng() % 40) - 20); if (rng() % 16 == 0) v = (rng() & 1) ? -0.0 : 0.0; }
  for (double& v : hq) v = val(rng);
  const double alpha0 = 1.0e9 * (1.0 + val(rng));
  Region ru_ = make_region(nc, gu, hq), rp_ = make_region(nc, gs, hq);
  const Region before = rp_;
  replay(pu, ru_, st, alpha0); replay(pp, rp_, st, alpha0);
  int diff = 0, pad_touched = 0;
  for (int i = 0; i < NC; ++i) for (int j = 0; j <= NC; ++j) {
    const double got = rp_.A()[i * (NC + 1) + j];
    const bool pad = i >= nc || (j >= nc && j < NC);
    if (pad) { if (!same_bits(got, before.d[(size_t)i * (NC + 1) + j])) ++pad_touched; }
    else if (!same_bits(got, ru_.A()[i * (nc + 1) + (j == NC ? nc : j)])) ++diff;
  }
  for (int i = 0; i < nc; ++i) for (int j = 0; j < NC; ++j) {
    const double got = rp_.Cm()[i * NC + j];
    if (j >= nc) { if (!same_bits(got, -0.0)) ++pad_touched; }
    else if (!same_bits(got, ru_.Cm()[i * nc + j])) ++diff;
  }
  for (int i = 0; i < 5 * nc; ++i) if (!same_bits(rp_.Cm()[rp_.nC() + i], ru_.Cm()[ru_.nC() + i])) ++diff;
  CHECK(diff == 0, "%s: %d real entries differ between the padded and the unpadded replay", name, diff);
  CHECK(pad_touched == 0, "%s: %d pad entries were written", name, pad_touched);
}

int main() {
  std::mt19937 rng(20260);
  // ---- which strides a circuit gets ----
  CHECK(persist_lu_nc(false, 0, 1) == 12 && persist_lu_nc(false, 0, 12) == 12 && persist_lu_nc(false, 0, 13) == 16 && persist_lu_nc(false, 0, 16) == 16, "register-LU size, narrow");
  CHECK(persist_lu_nc(true, 0, 3) == 16 && persist_lu_nc(false, 2, 9) == 16 && persist_lu_nc(false, 0, 17) == 0 && persist_lu_nc(true, 0, 17) == 0, "register-LU size, wide / bordered / too large");
  for (int nc = 1; nc <= 16; ++nc) for (int max_nc = nc; max_nc <= 16; ++max_nc) {
    const GatherStrides g = GatherStrides::of(false, 0, max_nc, nc), w = GatherStrides::of(true, 0, max_nc, nc), b = GatherStrides::of(false, 1, max_nc, nc);
    const int NC = max_nc <= 12 ? 12 : 16;
    CHECK(g.lda == NC + 1 && g.ldc == NC, "narrow nc %d of %d: strides %d %d", nc, max_nc, g.lda, g.ldc);
    CHECK(w.lda == 17 && w.ldc == 16, "wide nc %d: strides %d %d", nc, w.lda, w.ldc);
    CHECK(b.lda == nc + 1 && b.ldc == nc && b.extra_doubles(nc) == 0, "bordered nc %d: strides %d %d", nc, b.lda, b.ldc);
  }
  { const GatherStrides g = GatherStrides::of(false, 0, 40, 11); CHECK(g.lda == 12 && g.ldc == 11, "a circuit the device stepper does not take keeps the unpadded strides"); }
  CHECK((GatherStrides{13, 12}).extra_doubles(11) == 35, "the DFF tile pads 35 doubles");
  // ---- strides that cannot hold the class are refused ----
  {
    Class c = make_class(5, 5, 4, rng);
    GatherPlan gp;
    CHECK(!gp.build(5, c.mat_ptr, c.vec_ptr, c.src16, c.n_mat_src, GatherStrides{5, 5}), "lda == nc must be refused");
    CHECK(!gp.build(5, c.mat_ptr, c.vec_ptr, c.src16, c.n_mat_src, GatherStrides{6, 4}), "ldc < nc must be refused");
  }
  // ---- every block size under both register-LU sizes, a few densities each ----
  for (int NC : {12, 16}) for (int nc = 1; nc <= NC; ++nc) for (int rep = 0; rep < 4; ++rep) {
    const int dens = rep == 0 ? 10 : 1 + (int)(rng() % 9), heavy = 1 + (int)(rng() % 30);
    check_pair(make_class(nc, dens, heavy, rng), NC, ("nc " + std::to_string(nc) + " NC " + std::to_string(NC) + " rep " + std::to_string(rep)).c_str(), rng);
  }
  std::printf("gather strides: %d plans, %d bad\n", n_plans, n_bad);
  return n_bad == 0 ? 0 : 1;
}
