// Host-only test of cedarsim.jl_amd/csrc/ch_param_tables.hpp: the per-sample device tables built from a description and slot values
// (build_param_tables) and the partial copies a perturbed slot gets (perturb_tables).  The central property: the tables
// perturb_tables returns, resolved per flattened device and per sample through the indirections the kernels use, are bit-for-bit
// those of build_param_tables run again with the slot's values replaced.  Built with sanitizers by tests/test_host_param_tables.py.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "ch_param_tables.hpp"
using namespace chip;

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { if (nbad < 40) std::printf("line %d (%s): %s\n", __LINE__, g_case.c_str(), #c); ++nbad; } } while (0)
static std::string g_case = "-";

static const double k_default_card[CH_B4_NPAR] = {
#define P(n, d) d,
#define B(n, d) d, 0.0, 0.0, 0.0,
#define I(n)
#include "cedarhip_bsim4_params.def"
};

static bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

struct Circuit {
  Description D;
  std::vector<ClassMeta> cms;
  int add(int kind, int n0, int n1, int n2 = 0, int n3 = 0, double p0 = 1.0, int ip0 = 0) {
    HDev d = HDev();
    d.kind = kind; d.node[0] = n0; d.node[1] = n1; d.node[2] = n2; d.node[3] = n3; d.ipar[0] = ip0; d.mult = 1.0; d.va_nt = 4;
    for (int k = 0; k < CH_DEV_NPAR; ++k) d.par[k] = CH_NAN;
    d.par[0] = p0;
    D.dev.push_back(d);
    return (int)D.dev.size() - 1;
  }
  int mos(int nd, int ng, int ns, int nb, double w, double l) {
    const int i = add(CH_DEV_MOS, nd, ng, ns, nb, w, 0);
    D.dev[i].par[CH_MOS_L] = l; D.dev[i].par[CH_MOS_NF] = 1.0;
    return i;
  }
  int source(int kind, double dc) {
    HSource s; s.kind = kind; s.dc = dc; for (double& p : s.par) p = 0.0;
    if (kind == CH_SRC_DC) s.par[0] = dc; else { s.par[0] = 0.0; s.par[1] = 1e-6; s.par[2] = 1e-9; s.par[3] = 1e-10; s.par[4] = 1e-10; s.par[5] = 1e-8; s.par[6] = 2e-8; }
    D.src.push_back(s);
    return (int)D.src.size() - 1;
  }
  int slot(int kind, int a, int b = 0) { D.slot_kind.push_back(kind); D.slot_a.push_back(a); D.slot_b.push_back(b); return (int)D.slot_kind.size() - 1; }
  bool finish(int n_nodes) {
    D.n_nodes = n_nodes;
    std::vector<char> protect(D.dev.size(), 0), swept(D.src.size(), 1);
    if (analyse(n_nodes, D.dev, D.src, protect, swept, D.A) != CH_OK) return false;
    cms.resize(D.A.classes.size());
    for (size_t c = 0; c < cms.size(); ++c) { std::memset(&cms[c], 0, sizeof(ClassMeta)); cms[c].nc = D.A.classes[c].nc; cms[c].ndev = D.A.classes[c].ndev; cms[c].blob_ofs = 1000 + (int)c; }
    return true;
  }
};

// two blocks (nodes 2, 3 and nodes 4, 5) between ground and a supply on node 1; M0 and M1 have one geometry
struct Main : Circuit {
  int vdd, ipulse, r, c, m[4];
  Main() {
    D.model.push_back(std::vector<double>(k_default_card, k_default_card + CH_B4_NPAR));
    D.va_par = {1.5, 2.5};
    vdd = source(CH_SRC_DC, 1.75); ipulse = source(CH_SRC_PULSE, 0.25e-6);
    add(CH_DEV_V, 1, 0, 0, 0, 0.0, vdd);
    r = add(CH_DEV_R, 1, 2, 0, 0, 1000.0);
    m[0] = mos(2, 3, 0, 0, 1e-6, 0.5e-6);
    m[1] = mos(3, 2, 0, 0, 1e-6, 0.5e-6);
    c = add(CH_DEV_C, 3, 0, 0, 0, 1e-12);
    m[2] = mos(4, 5, 0, 0, 2e-6, 0.5e-6);
    m[3] = mos(5, 4, 1, 1, 1e-6, 0.75e-6);
    add(CH_DEV_I, 5, 0, 0, 0, 0.0, ipulse);
  }
};

struct Resolved {   // what the kernels would read for one sample
  std::vector<double> dpar, dmult, src_dc, src_par, vapar, col_dcls, col_block; double gmin, temp;
};
// base tables T with the override O on top (O = nullptr: T alone)
static Resolved resolve(const Description& D, const ParamTables& T, const TableOverride* O, int s) {
  const Analysis& A = D.A;
  auto lin = [&](int t) -> const std::vector<double>& { return O && !O->lin(t).empty() ? O->lin(t) : T.lin(t); };
  auto at = [&](int t, int S) { return S > 1 ? s : 0; };
  Resolved R;
  const size_t nh = D.dev.size(), nsrc = D.src.size(), nvp = std::max<size_t>(1, D.va_par.size());
  for (size_t d = 0; d < nh; ++d) { R.dpar.push_back(lin(LT_DPAR).at(d * T.Spar + at(0, T.Spar))); R.dmult.push_back(lin(LT_DMULT).at(d * T.Spar + at(0, T.Spar))); }
  for (size_t i = 0; i < nsrc; ++i) {
    R.src_dc.push_back(lin(LT_SRC_DC).at(at(0, T.Ssrc) * nsrc + i));
    for (size_t k = 0; k < CH_SRC_NPAR; ++k) R.src_par.push_back(lin(LT_SRC_PAR).at((at(0, T.Ssrc) * nsrc + i) * CH_SRC_NPAR + k));
  }
  for (size_t k = 0; k < nvp; ++k) R.vapar.push_back(lin(LT_VAPAR).at(at(0, T.Sva) * nvp + k));
  R.gmin = lin(LT_GMIN).at(at(0, T.Sgmin)); R.temp = lin(LT_TEMP).at(at(0, T.Stemp));
  const std::vector<double>& mosp = O && !O->mosp.empty() ? O->mosp : T.mosp;
  const std::vector<int>& dcls = O && !O->dcls.empty() ? O->dcls : T.dcls;
  const std::vector<int>& dl = O && !O->dcls_local.empty() ? O->dcls_local : T.dcls_local;
  const std::vector<int>& ml = O && !O->mc_list.empty() ? O->mc_list : T.mc_list;
  const std::vector<BlockMeta>& bm = O && !O->bmeta.empty() ? O->bmeta : T.bmeta;
  const long cols = O ? O->mos_cols : T.mos_cols(); const int ncls = O ? O->n_mos_cls : T.n_cls, max_mc = O ? O->max_mc : T.max_mc;
  CHECK(mosp.size() == (size_t)B4I_COUNT * cols + 2 && mosp[mosp.size() - 1] == 0.0 && mosp[mosp.size() - 2] == 0.0);   // the two padding doubles
  auto column = [&](int cl, std::vector<double>& out) {
    CHECK(cl >= 0 && cl < ncls);
    const long col = (long)cl * T.Smos + at(0, T.Smos);
    CHECK(col < cols);
    if (col < cols) out.insert(out.end(), mosp.begin() + col * B4I_COUNT, mosp.begin() + (col + 1) * B4I_COUNT);
  };
  for (int k = 0; k < A.n_comp; ++k) {
    const BlockMeta& b = bm.at(k);
    CHECK(b.uofs == A.comp_uofs[k] && b.dofs == A.comp_dofs[k] && b.mc_n <= max_mc && b.mc_ofs >= 0 && b.mc_ofs + b.mc_n <= (int)ml.size());
    for (int j = 0; j < b.mc_n && j < 8; ++j) CHECK(b.mc[j] == ml.at(b.mc_ofs + j));   // the inline mirror of the list
    for (int d = 0; d < A.comp_ndev[k]; ++d) {
      const int e = A.comp_dofs[k] + d;
      if (A.edev[e].mos < 0) continue;
      column(dcls.at(e), R.col_dcls);
      CHECK(dl.at(e) >= 0 && dl.at(e) < b.mc_n);
      column(ml.at(b.mc_ofs + dl.at(e)), R.col_block);
    }
  }
  return R;
}
static bool equal(const Resolved& a, const Resolved& b) {
  auto v = [](const std::vector<double>& x, const std::vector<double>& y) { return x.size() == y.size() && same_bits(x.data(), y.data(), x.size()); };
  return v(a.dpar, b.dpar) && v(a.dmult, b.dmult) && v(a.src_dc, b.src_dc) && v(a.src_par, b.src_par) && v(a.vapar, b.vapar) && v(a.col_dcls, b.col_dcls) &&
         v(a.col_block, b.col_block) && same_bits(&a.gmin, &b.gmin, 1) && same_bits(&a.temp, &b.temp, 1);
}

using Values = std::vector<std::vector<double>>;
static bool same_field(const Description& D, int i, int j) { return D.slot_kind[i] == D.slot_kind[j] && D.slot_a[i] == D.slot_a[j] && D.slot_b[i] == D.slot_b[j]; }

// perturb slot `id` on top of the slot values V and compare with the rebuild.  The perturbed slot wins over every set slot on its
// field, so the equivalent rebuild is the one in which all of them hold the new values.  `present`: the tables the override may hold.
enum { HAS_DPAR = 1, HAS_DMULT = 2, HAS_GMIN = 4, HAS_TEMP = 8, HAS_VAPAR = 16, HAS_SRC_DC = 32, HAS_SRC_PAR = 64, HAS_MOSP = 128, HAS_INST = 256 };
static void check_perturbation(const Circuit& C, const Values& V, int S, int id, unsigned present, bool va_setup) {
  const Description& D = C.D;
  std::string err;
  ParamTables T, R; TableOverride O;
  const SlotValues sl{D, V, S};
  CHECK(build_param_tables(D, sl, C.cms, T, err) == CH_OK);
  std::vector<double> val(S);
  for (int s = 0; s < S; ++s) { const double p = sl.value(id, s); val[s] = p != 0.0 ? p * (1.0 + 1.0 / 1024.0) : 1.0 / 1048576.0; }
  CHECK(perturb_tables(D, sl, T, id, val, O, err) == CH_OK);
  Values V2 = V;
  V2[id] = val;
  for (int j = 0; j < sl.count(); ++j) if (j != id && sl.is_set(j) && same_field(D, id, j)) V2[j] = val;
  CHECK(build_param_tables(D, SlotValues{D, V2, S}, C.cms, R, err) == CH_OK);
  for (int s = 0; s < S; ++s) CHECK(equal(resolve(D, T, &O, s), resolve(D, R, nullptr, s)));
  const unsigned got = (O.dpar.empty() ? 0 : HAS_DPAR) | (O.dmult.empty() ? 0 : HAS_DMULT) | (O.gmin.empty() ? 0 : HAS_GMIN) | (O.temp.empty() ? 0 : HAS_TEMP) |
                       (O.vapar.empty() ? 0 : HAS_VAPAR) | (O.src_dc.empty() ? 0 : HAS_SRC_DC) | (O.src_par.empty() ? 0 : HAS_SRC_PAR) | (O.mosp.empty() ? 0 : HAS_MOSP) |
                       (O.dcls.empty() ? 0 : HAS_INST);
  CHECK(got == present);
  CHECK(O.dcls.empty() == O.bmeta.empty() && O.dcls.empty() == O.mc_list.empty() && O.dcls.empty() == O.dcls_local.empty());
  CHECK(O.va_setup == va_setup);
  const bool inst = (present & HAS_INST) != 0;
  CHECK(O.n_mos_cls == T.n_cls + (inst ? 1 : 0) && O.mos_cols == (long)std::max(1, O.n_mos_cls) * T.Smos && O.max_mc == T.max_mc + (inst ? 1 : 0));
  CHECK(O.lds_extra_doubles == (inst ? (size_t)B4L_STRIDE : 0));
}

static void central_property() {
  Main C;
  struct K { int id, sibling; unsigned present; bool va; const char* name; };
  std::vector<K> kinds;
  auto two = [&](const char* name, unsigned present, bool va, int kind, int a, int b = 0) { const int i = C.slot(kind, a, b), j = C.slot(kind, a, b); kinds.push_back({i, j, present, va, name}); kinds.push_back({j, i, present, va, name}); };
  two("resistance", HAS_DPAR, false, CH_SLOT_DEV_PAR, C.r, 0);
  two("a field no linear device reads", 0, false, CH_SLOT_DEV_PAR, C.r, 1);
  two("capacitor multiplier", HAS_DMULT, false, CH_SLOT_DEV_MULT, C.c);
  two("MOSFET multiplier", HAS_DMULT, false, CH_SLOT_DEV_MULT, C.m[2]);
  two("W of a MOSFET in a shared class", HAS_MOSP | HAS_INST, false, CH_SLOT_DEV_PAR, C.m[0], CH_MOS_W);
  two("L of a MOSFET alone in its class", HAS_MOSP | HAS_INST, false, CH_SLOT_DEV_PAR, C.m[3], CH_MOS_L);
  two("card parameter", HAS_MOSP, false, CH_SLOT_MODEL_PAR, 0, CH_B4_vth0);
  two("DC value of a DC source", HAS_SRC_DC | HAS_SRC_PAR, false, CH_SLOT_SRC_DC, C.vdd);
  two("DC value of a pulse source", HAS_SRC_DC, false, CH_SLOT_SRC_DC, C.ipulse);
  two("pulse parameter", HAS_SRC_PAR, false, CH_SLOT_SRC_PAR, C.ipulse, 1);
  two("temperature", HAS_TEMP | HAS_MOSP, true, CH_SLOT_TEMP, 0);
  two("gmin", HAS_GMIN, false, CH_SLOT_GMIN, 0);
  two("Verilog-A parameter", HAS_VAPAR, true, CH_SLOT_VA_PAR, 1);
  const int bg_w = C.slot(CH_SLOT_DEV_PAR, C.m[2], CH_MOS_W), bg_r = C.slot(CH_SLOT_DEV_MULT, C.r);   // background: other fields, set per sample
  CHECK(C.finish(5));
  CHECK(C.D.A.n_comp == 2 && C.D.A.mos_hdev.size() == 4);
  const int nslot = (int)C.D.slot_kind.size();
  for (int S : {1, 3}) for (int background = 0; background < 2; ++background) for (const K& k : kinds) for (int state = 0; state < 3; ++state) {
    g_case = std::string(k.name) + (state == 0 ? ", unset" : state == 1 ? ", set" : ", sibling set") + (background ? ", other slots set" : "") + ", S = " + std::to_string(S);
    Values V(nslot);
    auto set = [&](int i, double rel) { V[i].resize(S); for (int s = 0; s < S; ++s) V[i][s] = slot_base(C.D, i) * (1.0 + rel * (s + 1)) + (slot_base(C.D, i) == 0.0 ? rel * (s + 1) : 0.0); };
    if (background) { set(bg_w, 1.0 / 64.0); set(bg_r, 1.0 / 32.0); }
    if (state == 1) set(k.id, 1.0 / 16.0);
    if (state == 2) set(k.sibling, 1.0 / 8.0);
    if (state == 1 && k.sibling > k.id) set(k.sibling, 1.0 / 4.0);   // (and a later slot on the field that would win in the tables)
    check_perturbation(C, V, S, k.id, k.present, k.va);
  }
  g_case = "-";
}

static void classes_and_layout() {
  Main C;
  const int w0 = C.slot(CH_SLOT_DEV_PAR, C.m[0], CH_MOS_W), w1 = C.slot(CH_SLOT_DEV_PAR, C.m[1], CH_MOS_W);
  CHECK(C.finish(5));
  const Description& D = C.D;
  std::string err;
  const int S = 3;
  ParamTables T;
  Values V(2);
  // identical instances share one class
  g_case = "identical instances";
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  CHECK(T.n_cls == 3 && T.mos_cls[0] == T.mos_cls[1] && T.mos_cls[2] != T.mos_cls[0] && T.mos_cls[3] != T.mos_cls[0] && T.mos_cls[3] != T.mos_cls[2]);
  CHECK(T.Smos == 1 && T.mosp.size() == (size_t)B4I_COUNT * 3 + 2 && T.cls_rep.size() == 3 && T.cls_rep[T.mos_cls[0]] == 0);
  CHECK(T.max_mc == 2 && T.mc_n[0] + T.mc_n[1] == (int)T.mc_list.size() && T.retained_bytes() > T.mosp.size() * sizeof(double));
  // equal per-sample overrides on two devices still share a class; unequal ones do not
  g_case = "equal overrides";
  V[w0] = {1.1e-6, 1.2e-6, 1.3e-6}; V[w1] = V[w0];
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  CHECK(T.n_cls == 3 && T.mos_cls[0] == T.mos_cls[1] && T.Smos == 3 && T.mosp.size() == (size_t)B4I_COUNT * 9 + 2);
  V[w1][2] = 1.4e-6;
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  CHECK(T.n_cls == 4 && T.mos_cls[0] != T.mos_cls[1]);
  // an instance slot on a shared class: one more column, the sibling's untouched
  g_case = "instance slot on a shared class";
  V[w0].clear(); V[w1].clear();
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  TableOverride O;
  CHECK(perturb_tables(D, SlotValues{D, V, S}, T, w0, {1.5e-6, 1.5e-6, 1.5e-6}, O, err) == CH_OK);
  CHECK(O.n_mos_cls == T.n_cls + 1 && O.mos_cols == 4 && O.mosp.size() == (size_t)B4I_COUNT * 4 + 2);
  CHECK(same_bits(O.mosp.data(), T.mosp.data(), (size_t)B4I_COUNT * 3));
  int e0 = -1, e1 = -1;
  for (size_t e = 0; e < D.A.edev.size(); ++e) { if (D.A.edev[e].mos == 0) e0 = (int)e; if (D.A.edev[e].mos == 1) e1 = (int)e; }
  CHECK(e0 >= 0 && e1 >= 0 && O.dcls[e0] == T.n_cls && O.dcls[e1] == T.dcls[e1] && O.dcls_local[e1] == T.dcls_local[e1]);
  CHECK(O.mosp[(size_t)B4I_COUNT * 3 + B4I_weff] != T.mosp[(size_t)B4I_COUNT * T.mos_cls[0] + B4I_weff]);
  // the sparse path reads dcls alone
  CHECK(perturb_tables(D, SlotValues{D, V, S}, T, w0, {1.5e-6, 1.5e-6, 1.5e-6}, O, err, false) == CH_OK);
  CHECK(!O.dcls.empty() && O.bmeta.empty() && O.mc_list.empty() && O.dcls_local.empty() && O.max_mc == T.max_mc && O.lds_extra_doubles == 0);
  // a zero channel length: the geometry error, from the builder and from a perturbation
  g_case = "zero channel length";
  const int l3 = (int)C.D.slot_kind.size();
  C.slot(CH_SLOT_DEV_PAR, C.m[3], CH_MOS_L);
  V.resize(3);
  err.clear();
  CHECK(perturb_tables(D, SlotValues{D, V, S}, T, l3, {0.0, 0.0, 0.0}, O, err) == CH_ERR_INVALID && err == "invalid MOS geometry or model card");
  V[l3] = {0.75e-6, 0.0, 0.75e-6};
  err.clear();
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_ERR_INVALID && err == "invalid MOS geometry or model card");
  // a sub-model the engine does not implement
  g_case = "unsupported sub-model";
  V[l3].clear();
  C.D.model[0][CH_B4_rdsmod] = 1.0;
  err.clear();
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_ERR_UNSUPPORTED && err.find("sub-model the engine does not implement") != std::string::npos);
  C.D.model[0][CH_B4_rdsmod] = 0.0;
  // a MOSFET the structural analysis does not hold: a slot on it reaches nothing
  g_case = "removed device";
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  const int ghost = C.mos(2, 3, 0, 0, 3e-6, 0.5e-6), wg = C.slot(CH_SLOT_DEV_PAR, ghost, CH_MOS_W);
  V.resize(wg + 1);
  CHECK(perturb_tables(D, SlotValues{D, V, S}, T, wg, {4e-6, 4e-6, 4e-6}, O, err) == CH_OK);
  CHECK(O.mosp.empty() && O.dcls.empty() && O.bmeta.empty() && O.dpar.empty() && O.n_mos_cls == T.n_cls && O.mos_cols == T.mos_cols() && O.lds_extra_doubles == 0);
  g_case = "-";
}

// n MOSFETs of n widths in one block: the list beyond the 8 inline entries, and the 64-class ceiling of the fused kernel
static void many_classes() {
  for (int n : {12, 63, 64}) {
    g_case = std::to_string(n) + " classes in a block";
    Circuit C;
    C.D.model.push_back(std::vector<double>(k_default_card, k_default_card + CH_B4_NPAR));
    C.add(CH_DEV_V, 1, 0, 0, 0, 0.0, C.source(CH_SRC_DC, 1.75));
    C.add(CH_DEV_R, 1, 2, 0, 0, 1000.0);
    std::vector<int> m;
    for (int i = 0; i < n; ++i) m.push_back(C.mos(2, 3, 0, 0, (1.0 + i / 64.0) * 1e-6, 0.5e-6));
    C.add(CH_DEV_C, 3, 0, 0, 0, 1e-12);
    const int w = C.slot(CH_SLOT_DEV_PAR, m[n - 1], CH_MOS_W);
    CHECK(C.finish(3));
    CHECK(C.D.A.n_comp == 1);
    Values V(1);
    if (n < 64) {
      for (int S : {1, 3}) check_perturbation(C, V, S, w, HAS_MOSP | HAS_INST, false);
      continue;
    }
    std::string err;
    ParamTables T; TableOverride O;
    const SlotValues sl{C.D, V, 1};
    CHECK(build_param_tables(C.D, sl, C.cms, T, err) == CH_OK);
    CHECK(T.n_cls == 64 && T.max_mc == 64 && T.bmeta[0].mc_n == 64);
    for (int j = 0; j < 8; ++j) CHECK(T.bmeta[0].mc[j] == T.mc_list[j]);
    CHECK(perturb_tables(C.D, sl, T, w, {3e-6}, O, err) == CH_ERR_UNSUPPORTED && err.find("64 MOSFET classes") != std::string::npos);
    CHECK(perturb_tables(C.D, sl, T, w, {3e-6}, O, err, false) == CH_OK && O.n_mos_cls == 65);
  }
  g_case = "-";
}

// the builder's own index conventions, against values written down here (the comparisons above go through slot_target on both sides)
static void absolute_layout() {
  g_case = "layout";
  Main C;
  const int sr = C.slot(CH_SLOT_DEV_PAR, C.r, 0), sm = C.slot(CH_SLOT_DEV_MULT, C.c), sv = C.slot(CH_SLOT_SRC_DC, C.vdd), si = C.slot(CH_SLOT_SRC_DC, C.ipulse);
  const int sp = C.slot(CH_SLOT_SRC_PAR, C.ipulse, 5), st = C.slot(CH_SLOT_TEMP, 0), sg = C.slot(CH_SLOT_GMIN, 0), sa = C.slot(CH_SLOT_VA_PAR, 1), sr2 = C.slot(CH_SLOT_DEV_PAR, C.r, 0);
  CHECK(C.finish(5));
  const Description& D = C.D;
  const int S = 3, nh = (int)D.dev.size();
  Values V(9);
  std::string err;
  ParamTables T;
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  CHECK(T.Spar == 1 && T.Ssrc == 1 && T.Smos == 1 && T.Sgmin == 1 && T.Stemp == 1 && T.Sva == 1);
  CHECK((int)T.dpar.size() == nh && T.dpar[C.r] == 1000.0 && T.dpar[C.c] == 1e-12 && T.dmult[C.c] == 1.0 && T.gmin == std::vector<double>{1e-12} && T.temp == std::vector<double>{27.0});
  CHECK(T.vapar == (std::vector<double>{1.5, 2.5}) && T.src_dc == (std::vector<double>{1.75, 0.25e-6}) && T.src_par.size() == 16 && T.src_par[0] == 1.75 && T.src_par[8 + 5] == 1e-8);
  V[sr] = {1.0, 2.0, 3.0}; V[sm] = {4.0, 5.0, 6.0}; V[sv] = {7.0, 8.0, 9.0}; V[si] = {10.0, 11.0, 12.0}; V[sp] = {13.0, 14.0, 15.0};
  V[st] = {16.0, 17.0, 18.0}; V[sg] = {19.0, 20.0, 21.0}; V[sa] = {22.0, 23.0, 24.0};
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  CHECK(T.Spar == 3 && T.Ssrc == 3 && T.Smos == 3 && T.Sgmin == 3 && T.Stemp == 3 && T.Sva == 3 && (int)T.dpar.size() == 3 * nh);
  for (int s = 0; s < S; ++s) {
    CHECK(T.dpar[C.r * 3 + s] == 1.0 + s && T.dpar[C.c * 3 + s] == 1e-12 && T.dmult[C.c * 3 + s] == 4.0 + s && T.dmult[C.r * 3 + s] == 1.0);
    CHECK(T.src_dc[s * 2 + C.vdd] == 7.0 + s && T.src_par[(s * 2 + C.vdd) * 8] == 7.0 + s);        // a DC source: the value is its first parameter as well
    CHECK(T.src_dc[s * 2 + C.ipulse] == 10.0 + s && T.src_par[(s * 2 + C.ipulse) * 8] == 0.0 && T.src_par[(s * 2 + C.ipulse) * 8 + 5] == 13.0 + s);
    CHECK(T.temp[s] == 16.0 + s && T.gmin[s] == 19.0 + s && T.vapar[s * 2 + 1] == 22.0 + s && T.vapar[s * 2] == 1.5);
    CHECK(T.mosp[((size_t)T.mos_cls[3] * 3 + s) * B4I_COUNT + B4I_vtm] == k::KboQ * ((16.0 + s) + 273.15));
  }
  V[sr2] = {31.0, 32.0, 33.0};   // a later slot on the same field wins
  CHECK(build_param_tables(D, SlotValues{D, V, S}, C.cms, T, err) == CH_OK);
  for (int s = 0; s < S; ++s) CHECK(T.dpar[C.r * 3 + s] == 31.0 + s);
  g_case = "-";
}

// SlotValues::value: the set value, else a set slot on the same field (the last one), else the base
static void slot_values() {
  Main C;
  const int a = C.slot(CH_SLOT_DEV_PAR, C.r, 0), b = C.slot(CH_SLOT_DEV_PAR, C.r, 0), c = C.slot(CH_SLOT_DEV_PAR, C.r, 0), t = C.slot(CH_SLOT_TEMP, 0), g = C.slot(CH_SLOT_GMIN, 0);
  const int v = C.slot(CH_SLOT_VA_PAR, 1), sd = C.slot(CH_SLOT_SRC_DC, C.vdd), sp = C.slot(CH_SLOT_SRC_PAR, C.ipulse, 5), mu = C.slot(CH_SLOT_DEV_MULT, C.c), mp = C.slot(CH_SLOT_MODEL_PAR, 0, CH_B4_capmod);
  CHECK(C.finish(5));
  Values V(10);
  const SlotValues sl{C.D, V, 2};
  CHECK(sl.value(a, 1) == 1000.0 && sl.value(t, 0) == 27.0 && sl.value(g, 1) == 1e-12 && sl.value(v, 0) == 2.5 && sl.value(sd, 0) == 1.75 && sl.value(sp, 0) == 1e-8);
  CHECK(sl.value(mu, 0) == 1.0 && sl.value(mp, 0) == 2.0 && slot_base(C.D, c) == 1000.0);
  V[b] = {1.0, 2.0};
  CHECK(sl.value(a, 1) == 2.0 && sl.value(b, 0) == 1.0 && sl.value(c, 0) == 1.0 && !sl.is_set(a) && sl.is_set(b));
  V[c] = {3.0, 4.0};
  CHECK(sl.value(a, 1) == 4.0 && sl.value(b, 1) == 2.0 && sl.value(t, 1) == 27.0);
}

int main() {
  slot_values();
  absolute_layout();
  central_property();
  classes_and_layout();
  many_classes();
  std::printf("param tables: %d checks, %d bad\n", nchecked, nbad);
  return nbad ? 1 : 0;
}
