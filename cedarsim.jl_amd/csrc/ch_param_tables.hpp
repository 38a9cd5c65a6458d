// ch_param_tables.hpp — "description + slot values -> per-sample device tables", HIP-free (plain g++ -std=c++17 compiles it;
// tests/host_param_tables.cpp runs it under ASan / UBSan).  build_param_tables makes every table finalize_params uploads;
// perturb_tables makes, for one slot taking other values, fresh copies of just the tables that slot reaches (the perturbed
// evaluations of ch_dc_sens).  Both go through the same writers, so each index convention is stated once:
//   slot_target       slot kind -> which linear table, which element per sample
//   mos_field         slot kind -> which part of a MOSFET's packed column
//   pack_mos_column   the override order (a later slot on the same field wins, the perturbed slot wins over all)
//   write_mos_class   class -> columns [cl * Smos + s] of mosp;  class_hdev: class -> representative instance
//   put_block_list    a block's class list: mc_list, BlockMeta::mc_ofs / mc_n and the inline mirror mc[j], j < 8
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/cedarhip.h"
#include "ch_analysis.hpp"
#include "ch_bsim4.hpp"

namespace chip {

// ---- description: filled by ch_circuit_build_impl, constant afterwards ----
struct Description {
  int n_nodes = 0; double temp = 27, gmin = 1e-12, scale = 1;
  std::vector<HDev> dev; std::vector<HSource> src; std::vector<std::vector<double>> model;
  std::vector<int> slot_kind, slot_a, slot_b, obs_kind, obs_index;
  std::vector<double> va_par;   // parameter blocks of the Verilog-A instances
  Analysis A;
};

struct ClassMeta {
  int nc, ndev, nonlinear, nslots;   // nslots: lane slots of the evaluation phase (4 per MOSFET, 1 otherwise)
  int wl_ofs, n_work, spare0, spare1;  // gather work list (register-LU variants): offset inside the blob (ints, even), items
  int n_mat_src, n_vec_src, blob_ofs, blob_ints;            // list lengths; this class's packed list blob (ints)
};

// Everything a block needs to address its data, in ONE 96-byte record (one dependent load level):
// offsets, a copy of its class record and (when they are at most 8) its MOS class ids.
struct BlockMeta {
  int uofs, dofs, mc_n, mc_ofs;
  ClassMeta cm;
  int mc[8];
};

// BSIM4 columns in LDS: one class per B4L_STRIDE doubles (even, so a column is a whole number of 16-byte pairs)
constexpr int B4L_STRIDE = (B4I_COUNT + 1) & ~1;

// ---- slots ----
// base value of slot i: what the description holds in the field the slot names
inline double slot_base(const Description& D, int i) {
  const int a = D.slot_a[i], b = D.slot_b[i];
  switch (D.slot_kind[i]) {
    case CH_SLOT_DEV_PAR: return D.dev[a].par[b];
    case CH_SLOT_DEV_MULT: return D.dev[a].mult;
    case CH_SLOT_MODEL_PAR: return D.model[a][b];
    case CH_SLOT_SRC_DC: return D.src[a].dc;
    case CH_SLOT_SRC_PAR: return D.src[a].par[b];
    case CH_SLOT_TEMP: return D.temp;
    case CH_SLOT_GMIN: return D.gmin;
    case CH_SLOT_VA_PAR: return D.va_par[a];
  }
  return 0.0;
}

// the slot values ch_set_params gave: val[i] is [S] or empty (slot not set)
struct SlotValues {
  const Description& D; const std::vector<std::vector<double>>& val; int S;
  int count() const { return (int)D.slot_kind.size(); }
  bool is_set(int i) const { return !val[i].empty(); }
  // value of slot i in sample s: what ch_set_params gave it, else the description's base value
  double value(int i, int s) const {
    if (is_set(i)) return val[i][s];
    // a second slot declared on the same field that does have values (the last one wins, as in the table builders)
    for (int j = count() - 1; j >= 0; --j)
      if (j != i && is_set(j) && D.slot_kind[j] == D.slot_kind[i] && D.slot_a[j] == D.slot_a[i] && D.slot_b[j] == D.slot_b[i]) return val[j][s];
    return slot_base(D, i);
  }
};

// ---- tables ----
// the tables a slot value lands in directly (everything but the packed MOSFET columns), and their layouts:
//   dpar, dmult [d * Spar + s]   gmin [s]   temp [s]   vapar [s * nvp + k]   src_dc [s * nsrc + i]   src_par [(s * nsrc + i) * CH_SRC_NPAR + k]
enum LinTab { LT_DPAR, LT_DMULT, LT_GMIN, LT_TEMP, LT_VAPAR, LT_SRC_DC, LT_SRC_PAR, LT_COUNT };
struct LinTables {
  std::vector<double> dpar, dmult, gmin, temp, vapar, src_dc, src_par;
  std::vector<double>& lin(int t) { std::vector<double>* const v[LT_COUNT] = {&dpar, &dmult, &gmin, &temp, &vapar, &src_dc, &src_par}; return *v[t]; }
  const std::vector<double>& lin(int t) const { return const_cast<LinTables*>(this)->lin(t); }
};

struct ParamTables : LinTables {
  int Spar = 1, Ssrc = 1, Smos = 1, Sgmin = 1, Stemp = 1, Sva = 1;   // samples each table holds: S, or 1 when no set slot reaches it
  int width(int t) const { const int w[LT_COUNT] = {Spar, Spar, Sgmin, Stemp, Sva, Ssrc, Ssrc}; return w[t]; }
  // MOSFET classes: instances with identical (model, geometry, overriding slots) share a column
  std::vector<int> mos_cls, cls_rep; int n_cls = 0;   // [n_mos] class of every instance; [n_cls] first instance of every class
  std::vector<double> mosp;                           // [n_cls * Smos][B4I_COUNT] + 2 doubles of padding (the kernel reads the columns in 16-byte pairs)
  std::vector<int> dcls;                              // [flattened device] class, 0 for other devices
  long mos_cols() const { return (long)std::max(1, n_cls) * Smos; }
  // per block: the distinct classes its devices use (mc_list[mc_ofs[k] .. + mc_n[k]]), and each device's index into that list
  std::vector<int> mc_ofs, mc_n, mc_list, dcls_local; std::vector<BlockMeta> bmeta; int max_mc = 0;
  size_t retained_bytes() const {
    size_t n = mosp.size() * sizeof(double) + bmeta.size() * sizeof(BlockMeta);
    for (int t = 0; t < LT_COUNT; ++t) n += lin(t).size() * sizeof(double);
    for (const std::vector<int>* v : {&mos_cls, &cls_rep, &dcls, &mc_ofs, &mc_n, &mc_list, &dcls_local}) n += v->size() * sizeof(int);
    return n;
  }
};

// What perturb_tables returns: fresh copies of the tables the slot reaches (a table it does not reach stays empty: the base's
// holds), and the scalars that go with them.
struct TableOverride : LinTables {
  std::vector<double> mosp; std::vector<int> dcls, dcls_local, mc_list; std::vector<BlockMeta> bmeta;
  long mos_cols = 0; int n_mos_cls = 0, max_mc = 0;
  size_t lds_extra_doubles = 0;   // what the fused kernel stages on top of the base tables' footprint
  bool va_setup = false;          // the Verilog-A constant blocks depend on a replaced table: they need a setup launch of their own
};

// Width groups: the tables that become per-sample when a slot is set.
enum : unsigned { SG_PAR = 1, SG_SRC = 2, SG_MOS = 4, SG_GMIN = 8, SG_TEMP = 16, SG_VA = 32 };
// Slot kind -> which table, which index: sample s of the slot is element ofs + s * step of table tab, for each of the n targets.
struct SlotTarget { unsigned groups = 0; int n = 0; struct { int tab; size_t ofs, step; } w[2]; };
inline SlotTarget slot_target(const Description& D, int Spar, int i) {
  const size_t a = (size_t)D.slot_a[i], b = (size_t)D.slot_b[i], nsrc = D.src.size(), nvp = std::max<size_t>(1, D.va_par.size());
  SlotTarget t;
  auto to = [&](int tab, size_t ofs, size_t step) { t.w[t.n].tab = tab; t.w[t.n].ofs = ofs; t.w[t.n].step = step; ++t.n; };
  switch (D.slot_kind[i]) {
    case CH_SLOT_DEV_PAR:
      if (D.dev[a].kind == CH_DEV_MOS) { t.groups = SG_MOS; break; }
      t.groups = SG_PAR; if (b == 0) to(LT_DPAR, a * Spar, 1);   // (no linear device reads another field)
      break;
    case CH_SLOT_DEV_MULT: t.groups = SG_PAR; to(LT_DMULT, a * Spar, 1); break;
    case CH_SLOT_MODEL_PAR: t.groups = SG_MOS; break;
    case CH_SLOT_SRC_DC:
      t.groups = SG_SRC; to(LT_SRC_DC, a, nsrc);
      if (D.src[a].kind == CH_SRC_DC) to(LT_SRC_PAR, a * CH_SRC_NPAR, nsrc * CH_SRC_NPAR);
      break;
    case CH_SLOT_SRC_PAR: t.groups = SG_SRC; to(LT_SRC_PAR, a * CH_SRC_NPAR + b, nsrc * CH_SRC_NPAR); break;
    case CH_SLOT_GMIN: t.groups = SG_GMIN; to(LT_GMIN, 0, 1); break;
    case CH_SLOT_TEMP: t.groups = SG_MOS | SG_TEMP; to(LT_TEMP, 0, 1); break;
    case CH_SLOT_VA_PAR: t.groups = SG_VA; to(LT_VAPAR, a, nvp); break;
  }
  return t;
}
// slot i takes v[s] in every sample the reached tables hold; table(tab) yields the vector to write
template <class Table> inline void write_slot(const Description& D, const ParamTables& W, int i, const double* v, Table&& table) {
  const SlotTarget t = slot_target(D, W.Spar, i);
  for (int k = 0; k < t.n; ++k) {
    std::vector<double>& dst = table(t.w[k].tab);
    for (int s = 0; s < W.width(t.w[k].tab); ++s) dst[t.w[k].ofs + (size_t)s * t.w[k].step] = v[s];
  }
}

// ---- MOSFET columns ----
// which part of MOSFET hd's column slot i sets
enum MosField { MF_NONE, MF_CARD, MF_INSTANCE, MF_TEMP };
inline MosField mos_field(const Description& D, int i, int hd) {
  if (D.slot_kind[i] == CH_SLOT_MODEL_PAR && D.slot_a[i] == D.dev[hd].ipar[0]) return MF_CARD;
  if (D.slot_kind[i] == CH_SLOT_DEV_PAR && D.slot_a[i] == hd) return MF_INSTANCE;
  if (D.slot_kind[i] == CH_SLOT_TEMP) return MF_TEMP;
  return MF_NONE;
}
// packed BSIM4 column of MOS device `hd` in sample s: card, geometry and temperature with every set slot applied.  pert_slot >= 0:
// that slot takes pert_value instead, set or not (the perturbed evaluations of ch_dc_sens)
inline int pack_mos_column(const Description& D, const SlotValues& sl, int hd, int s, int pert_slot, double pert_value, double* col, std::string& err) {
  std::vector<double> card = D.model[D.dev[hd].ipar[0]];
  double ip[CH_DEV_NPAR]; for (int k = 0; k < CH_DEV_NPAR; ++k) ip[k] = D.dev[hd].par[k];
  double tc = D.temp;
  auto apply = [&](int i, double v) {
    switch (mos_field(D, i, hd)) {
      case MF_CARD: card[D.slot_b[i]] = v; break;
      case MF_INSTANCE: ip[D.slot_b[i]] = v; break;
      case MF_TEMP: tc = v; break;
      case MF_NONE: break;
    }
  };
  for (int i = 0; i < sl.count(); ++i) if (sl.is_set(i) && i != pert_slot) apply(i, sl.val[i][s]);   // (s < Smos, and Smos = S when a slot that reaches a column is set)
  if (pert_slot >= 0) apply(pert_slot, pert_value);   // last: it wins over a set slot on the same field
  ip[CH_MOS_W] *= D.scale; ip[CH_MOS_L] *= D.scale;
  const int rc = b4_pack(card.data(), ip, tc, col);
  if (rc != CH_OK) err = rc == CH_ERR_UNSUPPORTED ? "BSIM4 card selects a sub-model the engine does not implement (rdsmod/rgatemod/rbodymod/igcmod/igbmod/trnqsmod/geomod != 0, diomod != 1, mobmod > 2, capmod not 0/2)" : "invalid MOS geometry or model card";
  return rc;
}
// the instance a class's columns are packed from: its first one
inline int class_hdev(const Description& D, const ParamTables& T, int cl) { return D.A.mos_hdev[T.cls_rep[cl]]; }
// columns [cl * Smos + s] of `table`, packed from device hd; pert_slot >= 0: with that slot at val[s]
inline int write_mos_class(const Description& D, const SlotValues& sl, int Smos, int cl, int hd, int pert_slot, const double* val, std::vector<double>& table, std::string& err) {
  double col[B4I_COUNT];
  for (int s = 0; s < Smos; ++s) {
    const int rc = pack_mos_column(D, sl, hd, s, pert_slot, pert_slot >= 0 ? val[s] : 0.0, col, err);
    if (rc != CH_OK) return rc;
    std::copy(col, col + B4I_COUNT, table.begin() + ((size_t)cl * Smos + s) * B4I_COUNT);
  }
  return CH_OK;
}
// a table of n_cols columns, with the padding behind it
inline std::vector<double> mos_table(long n_cols) { return std::vector<double>((size_t)B4I_COUNT * n_cols + 2, 0.0); }

// ---- block class lists ----
// block b's class list becomes `list`, appended to mc_list; the first 8 entries are mirrored in the record
inline void put_block_list(BlockMeta& b, std::vector<int>& mc_list, const std::vector<int>& list) {
  b.mc_ofs = (int)mc_list.size(); b.mc_n = (int)list.size();
  mc_list.insert(mc_list.end(), list.begin(), list.end());
  for (int j = 0; j < b.mc_n && j < 8; ++j) b.mc[j] = list[j];
}

// ---- all tables of a circuit: the host halves of finalize_params ----
inline int build_param_tables(const Description& D, const SlotValues& sl, const std::vector<ClassMeta>& class_metas, ParamTables& T, std::string& err) {
  const Analysis& A = D.A;
  const int nslot = sl.count(), S = sl.S, nh = (int)D.dev.size(), nsrc = (int)D.src.size();
  // which tables vary per sample
  unsigned set_groups = 0;
  for (int i = 0; i < nslot; ++i) if (sl.is_set(i)) set_groups |= slot_target(D, 1, i).groups;
  auto wide = [&](unsigned g) { return (set_groups & g) ? S : 1; };
  T.Spar = wide(SG_PAR); T.Ssrc = wide(SG_SRC); T.Smos = wide(SG_MOS); T.Sgmin = wide(SG_GMIN); T.Stemp = wide(SG_TEMP); T.Sva = wide(SG_VA);
  // linear device parameters and multipliers, sources, gmin, temperature and Verilog-A parameter blocks: base values, then the set slots in order
  T.dpar.resize((size_t)nh * T.Spar); T.dmult.resize((size_t)nh * T.Spar);
  for (int d = 0; d < nh; ++d) for (int s = 0; s < T.Spar; ++s) { T.dpar[(size_t)d * T.Spar + s] = D.dev[d].par[0]; T.dmult[(size_t)d * T.Spar + s] = D.dev[d].mult; }
  T.src_dc.assign((size_t)T.Ssrc * nsrc, 0.0); T.src_par.assign((size_t)T.Ssrc * nsrc * CH_SRC_NPAR, 0.0);
  for (int s = 0; s < T.Ssrc; ++s) for (int i = 0; i < nsrc; ++i) { T.src_dc[(size_t)s * nsrc + i] = D.src[i].dc; for (int k = 0; k < CH_SRC_NPAR; ++k) T.src_par[((size_t)s * nsrc + i) * CH_SRC_NPAR + k] = D.src[i].par[k]; }
  T.gmin.assign(T.Sgmin, D.gmin); T.temp.assign(T.Stemp, D.temp);
  const size_t nvp = std::max<size_t>(1, D.va_par.size());
  T.vapar.assign(nvp * T.Sva, 0.0);
  for (int s = 0; s < T.Sva; ++s) std::copy(D.va_par.begin(), D.va_par.end(), T.vapar.begin() + (size_t)s * nvp);
  for (int i = 0; i < nslot; ++i) if (sl.is_set(i)) write_slot(D, T, i, sl.val[i].data(), [&](int tab) -> std::vector<double>& { return T.lin(tab); });
  // MOS classes
  const int nmos = (int)A.mos_hdev.size();
  T.mos_cls.assign(nmos, 0); T.cls_rep.clear();
  std::map<std::vector<double>, int> cls_of;
  for (int m = 0; m < nmos; ++m) {
    const HDev& d = D.dev[A.mos_hdev[m]];
    std::vector<double> key;
    key.push_back(d.ipar[0]);
    for (int k = 0; k < 7; ++k) key.push_back(std::isnan(d.par[k]) ? -1e300 : d.par[k]);
    // an overriding slot: which field, and its values in every sample — instances whose overrides are EQUAL (a global W / L delta
    // of a Monte-Carlo sweep gives every device its own slot, but devices of one geometry the same values) still share a column
    for (int i = 0; i < nslot; ++i) if (sl.is_set(i) && D.slot_kind[i] == CH_SLOT_DEV_PAR && D.slot_a[i] == A.mos_hdev[m]) {
      key.push_back(1e6 + D.slot_b[i]);
      key.insert(key.end(), sl.val[i].begin(), sl.val[i].end());
    }
    auto it = cls_of.find(key);
    if (it == cls_of.end()) { it = cls_of.insert({key, (int)T.cls_rep.size()}).first; T.cls_rep.push_back(m); }
    T.mos_cls[m] = it->second;
  }
  T.n_cls = (int)T.cls_rep.size();
  T.mosp = mos_table(T.mos_cols());
  for (int cl = 0; cl < T.n_cls; ++cl) { const int rc = write_mos_class(D, sl, T.Smos, cl, class_hdev(D, T, cl), -1, nullptr, T.mosp, err); if (rc != CH_OK) return rc; }
  T.dcls.clear();
  for (const EDev& e : A.edev) T.dcls.push_back(e.mos >= 0 ? T.mos_cls[e.mos] : 0);
  // per block: the distinct MOS classes its devices use, and each device's index into that list
  // (a block with more than 64 distinct MOSFET classes takes the sparse path: the engine's path decision)
  T.mc_ofs.assign(A.n_comp, 0); T.mc_n.assign(A.n_comp, 0); T.mc_list.clear(); T.dcls_local.assign(A.edev.size(), 0); T.bmeta.resize(A.n_comp);
  T.max_mc = 0;
  for (int k = 0; k < A.n_comp; ++k) {
    std::vector<int> seen;
    for (int d = 0; d < A.comp_ndev[k]; ++d) {
      const EDev& e = A.edev[A.comp_dofs[k] + d];
      if (e.kind == K_VA) { T.dcls_local[A.comp_dofs[k] + d] = D.dev[e.hdev].ipar[0]; continue; }
      if (e.mos < 0) continue;
      const int cl = T.mos_cls[e.mos];
      const int j = (int)(std::find(seen.begin(), seen.end(), cl) - seen.begin());
      if (j == (int)seen.size()) seen.push_back(cl);
      T.dcls_local[A.comp_dofs[k] + d] = j;
    }
    BlockMeta& b = T.bmeta[k]; std::memset(&b, 0, sizeof(b));
    b.uofs = A.comp_uofs[k]; b.dofs = A.comp_dofs[k]; b.cm = class_metas[A.comp_class[k]];
    put_block_list(b, T.mc_list, seen);
    T.mc_ofs[k] = b.mc_ofs; T.mc_n[k] = b.mc_n;
    T.max_mc = std::max(T.max_mc, b.mc_n);
  }
  return CH_OK;
}

// ---- the tables of one perturbed evaluation: slot `id` takes val[s] in sample s, everything else stays ----
// `out` gets fresh copies of the tables the slot reaches, nothing else; the widths stay the base's, so a table that holds one sample
// takes val[0] (slot_value is the same in every sample then).  An instance parameter of a MOSFET gets a column of its own behind the
// table (class n_cls), since its class may be shared; block_lists: also one more entry in its block's class list, which the fused
// kernel stages (the sparse path reads dcls alone).
inline int perturb_tables(const Description& D, const SlotValues& sl, const ParamTables& T, int id, const std::vector<double>& val, TableOverride& out, std::string& err,
                          bool block_lists = true) {
  const Analysis& A = D.A;
  out = TableOverride();
  out.mos_cols = T.mos_cols(); out.n_mos_cls = T.n_cls; out.max_mc = T.max_mc;
  write_slot(D, T, id, val.data(), [&](int tab) -> std::vector<double>& { if (out.lin(tab).empty()) out.lin(tab) = T.lin(tab); return out.lin(tab); });
  const unsigned groups = slot_target(D, T.Spar, id).groups;
  out.va_setup = (groups & (SG_TEMP | SG_VA)) != 0;
  if (!(groups & SG_MOS)) return CH_OK;
  if (D.slot_kind[id] != CH_SLOT_DEV_PAR) {
    // a card parameter or the temperature: every class whose representative it reaches is packed again, in place
    bool any = false;
    for (int cl = 0; cl < T.n_cls; ++cl) {
      const int hd = class_hdev(D, T, cl);
      if (mos_field(D, id, hd) == MF_NONE) continue;
      if (!any) { out.mosp = T.mosp; any = true; }
      const int rc = write_mos_class(D, sl, T.Smos, cl, hd, id, val.data(), out.mosp, err);
      if (rc != CH_OK) return rc;
    }
    return CH_OK;
  }
  const int hd = D.slot_a[id];
  const int m = (int)(std::find(A.mos_hdev.begin(), A.mos_hdev.end(), hd) - A.mos_hdev.begin());
  if (m == (int)A.mos_hdev.size()) return CH_OK;   // the device was removed by the structural analysis
  out.mosp = mos_table((long)(T.n_cls + 1) * T.Smos);
  std::copy(T.mosp.begin(), T.mosp.begin() + (size_t)B4I_COUNT * T.n_cls * T.Smos, out.mosp.begin());
  const int rc = write_mos_class(D, sl, T.Smos, T.n_cls, hd, id, val.data(), out.mosp, err);
  if (rc != CH_OK) return rc;
  out.mos_cols = (long)(T.n_cls + 1) * T.Smos; out.n_mos_cls = T.n_cls + 1;
  int e = 0; while (e < (int)A.edev.size() && A.edev[e].mos != m) ++e;
  if (e == (int)A.edev.size()) return CH_OK;
  out.dcls = T.dcls; out.dcls[e] = T.n_cls;
  if (!block_lists) return CH_OK;
  int k = 0; while (!(e >= A.comp_dofs[k] && e < A.comp_dofs[k] + A.comp_ndev[k])) ++k;
  const BlockMeta& b0 = T.bmeta[k];
  if (b0.mc_n + 1 > 64) { err = "ch_dc_sens: a block with 64 MOSFET classes has no room for the perturbed instance's column"; return CH_ERR_UNSUPPORTED; }
  std::vector<int> list(T.mc_list.begin() + b0.mc_ofs, T.mc_list.begin() + b0.mc_ofs + b0.mc_n);
  list.push_back(T.n_cls);
  out.bmeta = T.bmeta; out.mc_list = T.mc_list; out.dcls_local = T.dcls_local;
  put_block_list(out.bmeta[k], out.mc_list, list);
  out.dcls_local[e] = b0.mc_n;
  out.max_mc = T.max_mc + 1; out.lds_extra_doubles = B4L_STRIDE;
  return CH_OK;
}

}  // namespace chip
