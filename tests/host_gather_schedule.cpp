// Host test of the gather schedule (cedarsim.jl_amd/csrc/ch_gather_plan.hpp), under ASan / UBSan (tests/test_host_gather_schedule.py).
// For every class: each item once, its sources in list order and contiguous in one lane, no lane above T, T within its bounds,
// every destination offset the one the work-list epilogue computes (r * lda + col / e), and a CPU replay of the kernel's trip loop
// (tran_persistent_kernel, ch_persist.hpp) on random stamp values equal (==, bit for bit) to the plain per-item sums for A, C, F, Q.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "ch_gather_plan.hpp"

using namespace chip;

static int n_bad = 0, n_classes = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++n_bad; std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

constexpr int CO = 16, QO = 4;   // StampLayout<false>: charge-Jacobian and charge offsets of a stamp record

struct Class {
  int nc = 0;
  std::vector<int> mat_ptr, vec_ptr;
  std::vector<uint16_t> src16;   // mat_src | vec_src
  int n_mat_src = 0;
};

// counts per matrix entry (nc * nc) and per row (nc) -> a class with random staging offsets
static Class make_class(int nc, const std::vector<int>& mat_cnt, const std::vector<int>& vec_cnt, std::mt19937& rng) {
  Class c; c.nc = nc;
  std::uniform_int_distribution<int> off(0, 1500);
  c.mat_ptr.push_back(0);
  for (int e = 0; e < nc * nc; ++e) { for (int k = 0; k < mat_cnt[e]; ++k) c.src16.push_back((uint16_t)off(rng)); c.mat_ptr.push_back((int)c.src16.size()); }
  c.n_mat_src = (int)c.src16.size();
  c.vec_ptr.push_back(0);
  for (int i = 0; i < nc; ++i) { for (int k = 0; k < vec_cnt[i]; ++k) c.src16.push_back((uint16_t)off(rng)); c.vec_ptr.push_back((int)c.src16.size() - c.n_mat_src); }
  return c;
}

static void check_class(const Class& c, const char* name, int expect_T, std::mt19937& rng) {
  ++n_classes;
  const int nc = c.nc, lda = nc + 1;
  GatherPlan gp;
  const bool built = gp.build(nc, c.mat_ptr, c.vec_ptr, c.src16, c.n_mat_src);
  CHECK(built, "%s: nc %d", name, nc);
  if (!built) return;
  // ---- the items, from the lists alone ----
  struct Ref { int first, cnt; bool vec; int e; };
  std::vector<Ref> ref;
  for (int i = 0; i < nc; ++i) ref.push_back({c.n_mat_src + c.vec_ptr[i], c.vec_ptr[i + 1] - c.vec_ptr[i], true, i});
  for (int e = 0; e < nc * nc; ++e) { const int cnt = c.mat_ptr[e + 1] - c.mat_ptr[e]; if (cnt > 0 || e / nc == e % nc) ref.push_back({c.mat_ptr[e], cnt, false, e}); }
  int total = 0, heaviest = 0;
  for (const Ref& r : ref) { const int s = r.cnt <= 0 ? 1 : (r.cnt + 3) / 4; total += s; heaviest = std::max(heaviest, s); }
  const int lb = std::max((total + 63) / 64, heaviest);
  CHECK(gp.n_items == (int)ref.size(), "%s: items %d, expected %zu", name, gp.n_items, ref.size());
  CHECK(gp.T >= lb, "%s: T %d below the bound %d", name, gp.T, lb);
  CHECK(gp.T <= (total + 63) / 64 + heaviest - 1, "%s: T %d above what first fit guarantees (%d trips, heaviest %d)", name, gp.T, total, heaviest);
  if (expect_T > 0) CHECK(gp.T == expect_T, "%s: T %d, expected %d", name, gp.T, expect_T);
  CHECK(gp.R >= total + 1 && gp.R < total + 5 && gp.R % 4 == 0 && (int)gp.words.size() == GP_HEAD_INTS + 3 * gp.R, "%s: %d records, %zu words", name, gp.R, gp.words.size());
  if ((int)gp.words.size() != GP_HEAD_INTS + 3 * gp.R) return;
  const int* head = gp.words.data(); const int* srcw = head + GP_HEAD_INTS; const int* ctlw = srcw + 2 * (size_t)gp.R;
  CHECK(srcw[0] == 0 && srcw[1] == 0 && ctlw[0] == 0, "%s: record 0 must idle", name);
  {   // the lanes' record ranges: inside the table, disjoint, none above T
    std::vector<int> owner(gp.R, -1);
    for (int l = 0; l < 64; ++l) {
      const int b = (int)((uint32_t)head[l] & 0xffffu), n = (int)((uint32_t)head[l] >> 16);
      CHECK(n <= gp.T, "%s: lane %d has %d trips, T %d", name, l, n, gp.T);
      CHECK(n == 0 || (b >= 1 && b + n <= gp.R), "%s: lane %d records %d + %d of %d", name, l, b, n, gp.R);
      if (!(n == 0 || (b >= 1 && b + n <= gp.R))) return;
      for (int q = 0; q < n; ++q) { CHECK(owner[b + q] < 0, "%s: record %d in two lanes", name, b + q); owner[b + q] = l; }
    }
  }
  // record of lane l at trip tr, as the kernel forms it
  auto rec_of = [&](int l, int tr) { const int b = (int)((uint32_t)head[l] & 0xffffu), n = (int)((uint32_t)head[l] >> 16); return tr < n ? b + tr : 0; };
  // ---- structure: walk every lane's trips; an item = the trips up to and including an END ----
  std::map<int, int> seen;   // destination key (vec: 0x10000 | e, else e) -> times
  int trips_used = 0;
  for (int l = 0; l < 64; ++l) {
    std::vector<uint16_t> acc; bool open = false, open_vec = false;
    for (int tr = 0; tr < gp.T; ++tr) {
      const int rec = rec_of(l, tr);
      const unsigned cw = (unsigned)ctlw[rec];
      const int n = (int)(cw & GP_N_MASK);
      const bool end = cw & GP_END, vec = cw & GP_VEC;
      CHECK(n <= 4, "%s: lane %d trip %d count %d", name, l, tr, n);
      if (cw == 0) { CHECK(!open, "%s: lane %d idles at trip %d inside an item", name, l, tr); continue; }
      ++trips_used;
      if (open) CHECK(vec == open_vec, "%s: lane %d trip %d changes kind inside an item", name, l, tr);
      if (!end) CHECK(n == 4, "%s: lane %d trip %d: %d sources in a trip that is not the item's last", name, l, tr, n);
      const uint32_t lo = (uint32_t)srcw[2 * rec], hi = (uint32_t)srcw[2 * rec + 1];
      const uint16_t o[4] = {(uint16_t)(lo & 0xffff), (uint16_t)(lo >> 16), (uint16_t)(hi & 0xffff), (uint16_t)(hi >> 16)};
      for (int k = 0; k < n; ++k) acc.push_back(o[k]);
      open = true; open_vec = vec;
      if (end) {
        const int oa = (int)((cw >> GP_A_SHIFT) & GP_OFS_MASK), oc = (int)(cw >> GP_C_SHIFT);
        int e = -1;
        if (vec) { e = oc - (nc * nc + 3 * nc); CHECK(e >= 0 && e < nc && oa == e * lda + nc, "%s: row item offsets %d %d", name, oa, oc); }
        else { e = oc; CHECK(e >= 0 && e < nc * nc && oa == (e / nc) * lda + e % nc, "%s: matrix item offsets %d %d", name, oa, oc); }
        ++seen[(vec ? 0x10000 : 0) | e];
        const Ref* r = nullptr;
        for (const Ref& q : ref) if (q.vec == vec && q.e == e) r = &q;
        CHECK(r != nullptr, "%s: lane %d closes an item that is not in the lists (vec %d e %d)", name, l, (int)vec, e);
        if (r) {
          CHECK((int)acc.size() == r->cnt, "%s: item (vec %d e %d) has %zu sources, expected %d", name, (int)vec, e, acc.size(), r->cnt);
          bool same = (int)acc.size() == r->cnt;
          for (int k = 0; same && k < r->cnt; ++k) same = acc[k] == c.src16[(size_t)r->first + k];
          CHECK(same, "%s: item (vec %d e %d): sources out of list order", name, (int)vec, e);
        }
        acc.clear(); open = false;
      }
    }
    CHECK(!open, "%s: lane %d ends inside an item", name, l);
  }
  CHECK(trips_used == total, "%s: %d trips in use, expected %d", name, trips_used, total);
  CHECK(seen.size() == ref.size(), "%s: %zu distinct items closed, expected %zu", name, seen.size(), ref.size());
  for (auto& kv : seen) CHECK(kv.second == 1, "%s: item %x closed %d times", name, kv.first, kv.second);
  // ---- replay of the kernel's trip loop against the plain per-item sums ----
  std::uniform_real_distribution<double> val(-1.0, 1.0);
  std::vector<double> st(1500 + CO + 1);
  for (double& v : st) { v = std::ldexp(val(rng), (int)(rng() % 40) - 20); if (rng() % 16 == 0) v = (rng() & 1) ? -0.0 : 0.0; }
  const double alpha0 = 1.0e9 * (1.0 + val(rng));
  const double SENT = 12345.678;
  const size_t nA = (size_t)nc * lda, nregion = nA + (size_t)nc * nc + 5 * (size_t)nc;   // A | Cm | xl xp Fv Qv hq
  std::vector<double> reg(nregion, SENT), exp_(nregion, SENT);
  double* A = reg.data(); double* Cm = A + nA; double* hq = Cm + (size_t)nc * nc + 4 * nc;
  for (int i = 0; i < nc; ++i) { hq[i] = val(rng); exp_[nA + (size_t)nc * nc + 4 * nc + i] = hq[i]; }
  {
    double s1[64], s2[64];
    for (int l = 0; l < 64; ++l) s1[l] = s2[l] = 0.0;
    for (int tr = 0; tr < gp.T; ++tr) for (int l = 0; l < 64; ++l) {
      const int rec = rec_of(l, tr);
      const uint32_t ox = (uint32_t)srcw[2 * rec], oy = (uint32_t)srcw[2 * rec + 1]; const unsigned cw = (unsigned)ctlw[rec];
      const int n = (int)(cw & GP_N_MASK);
      const bool vec = cw & GP_VEC;
      const int off2 = vec ? QO : CO;
      const int o0 = (int)(ox & 0xffffu), o1 = (int)(ox >> 16), o2 = (int)(oy & 0xffffu), o3 = (int)(oy >> 16);
      const int oa = (int)((cw >> GP_A_SHIFT) & GP_OFS_MASK), oc = (int)(cw >> GP_C_SHIFT);
      const double a0 = st[o0], b0 = st[o0 + off2], a1 = st[o1], b1 = st[o1 + off2], a2 = st[o2], b2 = st[o2 + off2], a3 = st[o3], b3 = st[o3 + off2];
      const double hqe = Cm[oc + nc];
      if (n > 0) { s1[l] += a0; s2[l] += b0; }
      if (n > 1) { s1[l] += a1; s2[l] += b1; }
      if (n > 2) { s1[l] += a2; s2[l] += b2; }
      if (n > 3) { s1[l] += a3; s2[l] += b3; }
      if (cw & GP_END) {
        const double G = s1[l] + alpha0 * s2[l];
        if (vec) { const double F = G + hqe; Cm[oc - nc] = F; A[oa] = -F; }
        else A[oa] = G;
        Cm[oc] = s2[l];
        s1[l] = 0.0; s2[l] = 0.0;
      }
    }
  }
  {   // the work-list epilogue, item by item
    double* eA = exp_.data(); double* eC = eA + nA; double* eF = eC + (size_t)nc * nc + 2 * nc; double* eQ = eF + nc;
    for (const Ref& r : ref) {
      double s1 = 0.0, s2 = 0.0;
      for (int k = 0; k < r.cnt; ++k) { const int o = c.src16[(size_t)r.first + k]; s1 += st[o]; s2 += st[o + (r.vec ? QO : CO)]; }
      if (r.vec) { eQ[r.e] = s2; const double F = s1 + alpha0 * s2 + hq[r.e]; eF[r.e] = F; eA[r.e * lda + nc] = -F; }
      else { const int row = r.e / nc, col = r.e - row * nc; eA[row * lda + col] = s1 + alpha0 * s2; eC[r.e] = s2; }
    }
  }
  int diff = 0;
  for (size_t i = 0; i < nregion; ++i) if (std::memcmp(&reg[i], &exp_[i], sizeof(double)) != 0) { if (!diff) std::printf("%s: first difference at region offset %zu: %.17g vs %.17g\n", name, i, reg[i], exp_[i]); ++diff; }
  CHECK(diff == 0, "%s: %d entries of A | C | F | Q differ between the replay and the per-item sums", name, diff);
}

int main() {
  std::mt19937 rng(20250);
  // ---- the DFF class: 59 structural non-zeros and 11 rows with 12, 12, 8 x 6, 6 x 8, 4 x 4, 2 x 26, 1 x 24 sources: T = 3 ----
  {
    const int nc = 11;
    std::vector<int> cnts = {12, 12};
    for (int i = 0; i < 6; ++i) cnts.push_back(8);
    for (int i = 0; i < 8; ++i) cnts.push_back(6);
    for (int i = 0; i < 4; ++i) cnts.push_back(4);
    for (int i = 0; i < 26; ++i) cnts.push_back(2);
    for (int i = 0; i < 24; ++i) cnts.push_back(1);
    std::shuffle(cnts.begin(), cnts.end(), rng);
    std::vector<int> mat(nc * nc, 0), vec(nc, 0);
    size_t k = 0;
    for (int i = 0; i < nc; ++i) vec[i] = cnts[k++];
    for (int i = 0; i < nc; ++i) mat[i * nc + i] = cnts[k++];            // every diagonal
    for (int e = 0; e < nc * nc && k < cnts.size(); ++e) if (mat[e] == 0 && (e * 7) % 3 != 0) mat[e] = cnts[k++];
    if (k != cnts.size()) { std::printf("FAIL: DFF class construction\n"); return 1; }
    check_class(make_class(nc, mat, vec, rng), "dff", 3, rng);
  }
  // ---- all light: T = 1 (and a diagonal without any source) ----
  for (int nc : {1, 8, 11, 12, 16}) {
    std::vector<int> mat(nc * nc, 0), vec(nc, 1);
    for (int i = 0; i < nc; ++i) mat[i * nc + i] = i == 0 ? 0 : 1 + i % 4;
    for (int i = 0; i + 1 < nc; ++i) mat[i * nc + i + 1] = 1;
    check_class(make_class(nc, mat, vec, rng), ("light nc " + std::to_string(nc)).c_str(), nc + nc + (nc - 1) <= 64 ? 1 : 0, rng);
  }
  // ---- one item heavier than everything else together ----
  for (int nc : {1, 8, 12}) {
    std::vector<int> mat(nc * nc, 0), vec(nc, 1);
    for (int i = 0; i < nc; ++i) mat[i * nc + i] = 1;
    mat[0] = 4 * (2 * nc) + 3;
    check_class(make_class(nc, mat, vec, rng), ("heavy nc " + std::to_string(nc)).c_str(), 2 * nc + 1, rng);
  }
  // ---- more than 128 items: all light (T = ceil(items / 64)), and mixed ----
  for (int nc : {12, 16}) {
    std::vector<int> mat(nc * nc, 1), vec(nc, 2);
    check_class(make_class(nc, mat, vec, rng), ("dense light nc " + std::to_string(nc)).c_str(), (nc * nc + nc + 63) / 64, rng);
    for (int e = 0; e < nc * nc; ++e) mat[e] = 1 + (e * 5) % 9;
    vec.assign(nc, 17);
    check_class(make_class(nc, mat, vec, rng), ("dense mixed nc " + std::to_string(nc)).c_str(), 0, rng);
  }
  // ---- random classes ----
  const int ncs[] = {1, 2, 3, 5, 8, 11, 12, 13, 16, 24, 32, 64};
  for (int rep = 0; rep < 300; ++rep) {
    const int nc = ncs[rng() % (sizeof(ncs) / sizeof(ncs[0]))];
    const int dens = 1 + (int)(rng() % 9), heavy = 1 + (int)(rng() % 30);
    std::vector<int> mat(nc * nc, 0), vec(nc, 0);
    for (int e = 0; e < nc * nc; ++e) if ((int)(rng() % 10) < dens) mat[e] = (rng() % 8 == 0) ? 1 + (int)(rng() % heavy) : 1 + (int)(rng() % 3);
    for (int i = 0; i < nc; ++i) vec[i] = (int)(rng() % (heavy + 1));
    check_class(make_class(nc, mat, vec, rng), ("random " + std::to_string(rep)).c_str(), 0, rng);
  }
  // ---- a class that does not fit the one-wave path ----
  {
    GatherPlan gp;
    std::vector<int> mp(65 * 65 + 1, 0), vp(66, 0);
    CHECK(!gp.build(65, mp, vp, {}, 0), "nc 65 must be refused");
  }
  std::printf("gather schedule: %d classes, %d bad\n", n_classes, n_bad);
  return n_bad == 0 ? 0 : 1;
}
