// ch_engine.hip — host side of the engine: contexts, circuits, parameter tables, the sequential
// adaptive time stepper and the C-ABI of include/cedarhip.h.
//
// Division of labour (BASELINE.json north_star): the outer adaptive time stepper and all one-off
// analysis stay on the host; every Newton solve runs on the GPU (ch_kernels.hpp).  Per step
// attempt the host (1) evaluates the source waveforms at t_new and uploads the few known-node /
// source values, (2) launches ONE fused Newton kernel + a tiny reduction, (3) reads back a 64-byte
// summary (converged?, iterations, local-error norms for orders k-1,k,k+1) and decides
// accept/reject, next step and next order — the job IDA does in the reference (src/sweeps.jl:456).
// There is NO CPU fallback: without a HIP device ch_create fails.
//
// One translation unit.  ch_circuit's state is grouped by owner, each group declared once in front of ch_circuit: Description (ch_param_tables.hpp; filled by
// ch_circuit_build_impl, then constant), Structure (uploaded once by upload_structure), SampleTables (rebuilt by finalize_params when
// dirty: the HIP-free build_param_tables of ch_param_tables.hpp, kept on the host beside the uploaded copies), NewtonState (rings, launch scratch, argument template), SparsePath (ch_engine_sparse.hpp, its decisions in the HIP-free ch_sparse_newton.hpp),
// DeviceStepper and TornCompanion (ch_engine_persist.hpp), SmallSignal (ch_engine_ac.hpp), Sensitivity (ch_engine_sens.hpp; the transient sensitivities of ch_engine_transens.hpp keep their state in a TranSens per call) and LaunchStats (HIP-free, ch_stepper_host.hpp).
// This file holds the context, those groups, the Newton launch and the C-ABI wrappers; the DC operating point is in ch_engine_dc.hpp, the
// transient driver and the host stepper's launch loop in ch_engine_tran.hpp; the waveform measurements over a finished transient in ch_engine_measure.hpp, the frequency-domain ones in ch_engine_fmeasure.hpp; ch_engine_diag.hpp has the benchmarks and test hooks.  Memory ownership is in ch_device_mem.hpp, the HIP-free step
// controller and source model in ch_stepper_host.hpp, the DC start vector and its generator in ch_dc_start.hpp, the environment switches in ch_env.hpp.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <new>
#include <stdexcept>
#include <string>
#include <array>
#include <vector>

#include "../../include/cedarhip.h"
#include "ch_analysis.hpp"
#include "ch_bsim4.hpp"
#include "ch_dc_start.hpp"
#include "ch_device_mem.hpp"
#include "ch_env.hpp"
#include "ch_gather_plan.hpp"
#include "ch_kernels.hpp"
#include "ch_noise_params.hpp"
#include "ch_param_tables.hpp"
#include "ch_persist.hpp"
#include "ch_sparse.hpp"
#include "ch_sens_host.hpp"
#include "ch_acsens_host.hpp"
#include "ch_noisesens_host.hpp"
#include "ch_sparse_newton.hpp"
#include "ch_stepper_host.hpp"
#include "ch_transens_host.hpp"
#include "ch_transens_kernels.hpp"
#include "ch_measure_kernels.hpp"
#include "ch_noisesens_kernels.hpp"
#include "ch_fmeasure_kernels.hpp"
#include "ch_loopgain_kernels.hpp"
#include "ch_netparams_kernels.hpp"

using namespace chip;
using hclock = std::chrono::steady_clock;

struct ch_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
};

struct ch_result {
  std::vector<double> times, values, final_state;
  std::vector<int32_t> pts;   // per saved row: newest saved points (this row included) the step's dense-output polynomial runs through; 0 = none
  const double* dev_values = nullptr; int64_t dev_n = 0;   // the same values still in HBM ([n_obs][n_times][n_samples]), owned by the circuit, or null
  ch_stats stats;
  int status = CH_OK;
  int n_obs = 0, S = 1;
  std::vector<double> sens; int n_par = 0;   // ch_tran_sens: d(observable)/d p_k as [n_obs][n_par][n_times][n_samples]
  ch_ctx* ctx = nullptr;                     // the context of the circuit that made it (ch_result_measure launches on its stream)
};

struct PersistConsts; struct PersistIo; struct PersistLaunch; struct PersistRun; struct PersistStep;   // ch_engine_persist.hpp
struct RowStore;   // ch_engine_tran.hpp
struct TranSens;   // ch_engine_transens.hpp
struct ch_circuit;

// ch_circuit's state, grouped by who writes it and when.  Every group that holds device or pinned memory is a member declared
// behind the arena.  A function that reads a few fields of another group names the group at the use (sp.Aval).
// ---- description (filled by ch_circuit_build_impl, constant afterwards): Description, ch_param_tables.hpp ----
// ---- structure: built and uploaded once by upload_structure ----
struct Structure {
  DevBuf<int> d_comp_class, d_comp_uofs, d_comp_dofs, d_gl_ptr, d_dkind, d_dterm, d_dsrc, d_dhdev, d_obs_unk, d_unk_obs;
  DevBuf<unsigned long long> d_stamps; DevBuf<ClassMeta> d_classes; DevBuf<unsigned char> d_dmask;
  DevBuf<int> d_dvac, d_va_mod, d_va_pofs, d_va_cofs;   // constant blocks of the Verilog-A instances: offset per flattened device; setup work list
  int n_va_inst = 0; size_t vac_total = 0; std::vector<ClassMeta> h_cms;
  std::vector<int> obs_primary;  // per observable: the observable whose device row it shares (itself if primary)
  std::vector<int> needed_src;   // sources that define a known node or feed a surviving device (others, e.g. merged 0 V ammeters, are never evaluated)
  std::vector<int> dev_src;      // sources whose value the kernels read (referenced by a surviving V / I device)
  int n_dev_src() const { return std::max<int>(1, (int)dev_src.size()); }
  int block_threads = 64, lu_variant = 16;
  bool wide_split = false; int wide_l = 0, wide_other = 0;   // class 0: its large compiled devices are evaluated in two halves; lanes per half; unsplit slots
  size_t lds_doubles_fixed = 0, lds_extra_bytes = 0, lds_plan_bytes = 0, lds_pad_doubles = 0;
  // the host-side steps of ch_circuit::upload_structure, in its order; the uploads between them stay there (they report through the context)
 private: friend struct ch_circuit;
  // class blobs: per class the gather pointers, lane slots, packed sources and register-LU work list -> h_cms, blob; launch shape
  void class_blobs(const Description& D, std::vector<int>& blob) {
    h_cms.clear();
    int max_slots = 0;
    for (size_t ci = 0; ci < D.A.classes.size(); ++ci) {
      const CompClass& c = D.A.classes[ci];
      ClassMeta m; std::memset(&m, 0, sizeof(m));
      m.nc = c.nc; m.ndev = c.ndev; m.nonlinear = c.nonlinear ? 1 : 0;
      m.n_mat_src = (int)c.mat_src.size(); m.n_vec_src = (int)c.vec_src.size();
      // one contiguous blob per class, copied verbatim into LDS: mat_ptr | vec_ptr | slots | mat_src | vec_src
      while (blob.size() & 3) blob.push_back(0);   // class blobs start on 16-byte boundaries (the kernel copies them with 16-byte loads)
      m.blob_ofs = (int)blob.size();
      blob.insert(blob.end(), c.mat_ptr.begin(), c.mat_ptr.end());
      blob.insert(blob.end(), c.vec_ptr.begin(), c.vec_ptr.end());
      int rep = -1;
      for (int k = 0; k < D.A.n_comp; ++k) if (D.A.comp_class[k] == (int)ci) { rep = k; break; }
      int ns = 0;
      // lane slots, expensive devices first so that they share wavefronts: compiled Verilog-A devices take one lane
      // per unknown terminal (direction-parallel duals: lane j computes column j of the stamp Jacobians; derivatives
      // with respect to known nodes are never gathered), MOSFETs and all other devices one lane each
      // A block whose compiled devices are large models (BSIM-CMG class) evaluates them in two halves on separate wavefronts:
      // bit 29 of a slot = split, bit 30 = which half (0: resistive sums and dI/dV, 1: charge sums and dQ/dV); the first halves
      // fill whole wavefronts (padded with idle slots) so that a wavefront never runs both code paths
      {
        std::vector<int> lanes;
        bool big = false;
        for (int d = 0; d < c.ndev; ++d) {
          const EDev& e = D.A.edev[D.A.comp_dofs[rep] + d];
          if (e.kind != K_VA) continue;
          if (va_gen::MODULES[D.dev[e.hdev].ipar[0]].n_params >= 64) big = true;
          bool first = true;
          for (int j = 0; j < e.nt; ++j) if (e.term[j] >= 0) { lanes.push_back((d << 4) | (first ? 8 : 0) | j); first = false; }
        }
        const bool split = big && !env_on(Env::VA_NOSPLIT);
        if (ci == 0) { wide_split = split; wide_l = (int)lanes.size(); wide_other = 0; }
        if (!split) { for (int v : lanes) { blob.push_back(v); ++ns; } }
        else {
          for (int v : lanes) { blob.push_back(v | (1 << 29)); ++ns; }
          while (ns & 63) { blob.push_back(-1); ++ns; }
          for (int v : lanes) { blob.push_back(v | (1 << 29) | (1 << 30)); ++ns; }
        }
      }
      for (int d = 0; d < c.ndev; ++d) if (D.A.edev[D.A.comp_dofs[rep] + d].kind == K_MOS) { blob.push_back(d << 4); ++ns; if (ci == 0) ++wide_other; }
      for (int d = 0; d < c.ndev; ++d) { const int kd = D.A.edev[D.A.comp_dofs[rep] + d].kind; if (kd != K_MOS && kd != K_VA) { blob.push_back(d << 4); ++ns; if (ci == 0) ++wide_other; } }
      m.nslots = ns;
      std::vector<uint16_t> h16(c.mat_src); h16.insert(h16.end(), c.vec_src.begin(), c.vec_src.end());
      if (h16.size() & 1) h16.push_back(0);
      for (size_t i = 0; i < h16.size(); i += 2) blob.push_back((int)((uint32_t)h16[i] | ((uint32_t)h16[i + 1] << 16)));
      // gather work list of the register-LU variants: structural non-zeros of A/C and all diagonals, then the rows of F/Q;
      // item = {first source (index into mat_src|vec_src), (sources << 16) | vector flag << 15 | entry}
      if (((int)blob.size() - m.blob_ofs) & 1) blob.push_back(0);
      m.wl_ofs = (int)blob.size() - m.blob_ofs;
      if (c.nc <= 64 && !c.vec_ptr.empty()) {
        // heaviest items first: when there are more items than lanes, the second pass of a wave holds only the lightest ones
        std::vector<std::array<int, 3>> items;   // {sources, first source, code}
        for (int i = 0; i < c.nc; ++i) {
          const int start = c.vec_ptr[i], cnt = c.vec_ptr[i + 1] - start;
          items.push_back({cnt, m.n_mat_src + start, (int)(0x8000u | (uint32_t)i)});
        }
        for (int e = 0; e < c.nc * c.nc; ++e) {
          const int start = c.mat_ptr[e], cnt = c.mat_ptr[e + 1] - start;
          if (cnt == 0 && e / c.nc != e % c.nc) continue;
          items.push_back({cnt, start, e});
        }
        std::stable_sort(items.begin(), items.end(), [](const std::array<int, 3>& x, const std::array<int, 3>& y) { return x[0] > y[0]; });
        for (const auto& it : items) { blob.push_back(it[1]); blob.push_back((int)(((uint32_t)it[0] << 16) | (uint32_t)it[2])); ++m.n_work; }
      }
      while ((blob.size() - m.blob_ofs) & 3) blob.push_back(0);
      m.blob_ints = (int)blob.size() - m.blob_ofs;
      // lane schedule of the device-resident stepper's gather (ch_gather_plan.hpp), directly BEHIND the blob (spare0 = its ints,
      // spare1 = trips): blob_ints stays what newton_block_kernel copies (its fast path and its LDS size depend on it);
      // tran_persistent_kernel copies blob_ints + spare0.  Its destination offsets follow the strides of that kernel's images of A
      // and C: padded to its register-LU size except in the bordered form (GatherStrides).
      if (m.n_work > 0) {
        GatherPlan gp;
        if (gp.build(c.nc, c.mat_ptr, c.vec_ptr, h16, m.n_mat_src, GatherStrides::of(D.A.wide, D.A.nb, D.A.max_nc, c.nc))) {
          m.spare0 = (int)gp.words.size(); m.spare1 = gp.T;
          blob.insert(blob.end(), gp.words.begin(), gp.words.end());
        }
      }
      if (env_on(Env::DEBUG_BLOB)) std::fprintf(stderr, "[blob] class %zu: nc %d ndev %d slots %d mat_src %d vec_src %d work %d blob_ints %d trips %d\n", ci, m.nc, m.ndev, m.nslots, m.n_mat_src, m.n_vec_src, m.n_work, m.blob_ints, m.spare1);
      max_slots = std::max(max_slots, m.nslots);
      h_cms.push_back(m);
    }
    block_threads = std::min(256, std::max(64, ((max_slots + 63) / 64) * 64));
    lu_variant = D.A.max_nc <= 8 ? 8 : (D.A.max_nc <= 12 ? 12 : (D.A.max_nc <= 16 ? 16 : (D.A.max_nc <= 32 ? 32 : 0)));
    if (D.A.wide) lu_variant = D.A.max_nc <= 16 ? 16 : 0;  // wide (Verilog-A) stamp records: two instantiations only
  }
  // per flattened device: kind, terminals, host device, source slot; the sources the kernels read and the ones ever evaluated
  void source_lists(const Description& D, std::vector<int>& dkind, std::vector<int>& dterm, std::vector<int>& dhdev, std::vector<int>& dsrc) {
    dsrc.clear();
    dev_src.clear();
    { std::vector<int> slot_of(D.src.size(), -1);
      for (const EDev& e : D.A.edev) {
        dkind.push_back(e.kind); for (int k = 0; k < NTERM; ++k) dterm.push_back(e.term[k]); dhdev.push_back(e.hdev);
        int si = e.kind == K_VA ? D.dev[e.hdev].ipar[1] : 0;
        if (e.src >= 0) { if (slot_of[e.src] < 0) { slot_of[e.src] = (int)dev_src.size(); dev_src.push_back(e.src); } si = slot_of[e.src]; }
        dsrc.push_back(si);
      }
      std::vector<char> need(D.src.size(), 0);
      for (int si : dev_src) need[si] = 1;
      for (const KnownDef& kd : D.A.known) for (auto& tm : kd.terms) need[tm.first] = 1;
      needed_src.clear();
      for (size_t i = 0; i < D.src.size(); ++i) if (need[i]) needed_src.push_back((int)i); }
  }
  // constant blocks (va_gen::setup) of the compiled Verilog-A instances
  void va_offsets(const Description& D, std::vector<int>& dvac, std::vector<int>& vmod, std::vector<int>& vpofs, std::vector<int>& vcofs) {
    dvac.assign(D.A.edev.size(), 0);
    vac_total = 0;
    for (size_t i = 0; i < D.A.edev.size(); ++i) {
      const EDev& e = D.A.edev[i];
      if (e.kind != K_VA) continue;
      const int mod = D.dev[e.hdev].ipar[0];
      dvac[i] = (int)vac_total; vmod.push_back(mod); vpofs.push_back(D.dev[e.hdev].ipar[1]); vcofs.push_back((int)vac_total);
      vac_total += (size_t)va_gen::N_CACHE[mod];
    }
    n_va_inst = (int)vmod.size();
    if (vmod.empty()) { vmod.push_back(0); vpofs.push_back(0); vcofs.push_back(0); }
  }
  void masks_and_observables(const Description& D, std::vector<unsigned char>& dm, std::vector<int>& obs_unk, std::vector<int>& unk_obs) {
    dm.assign(D.A.n_unk, 0);
    for (int u = 0; u < D.A.n_unk; ++u) dm[u] = (D.A.diff_mask[u] ? 1 : 0) | (D.A.unk_mna[u] >= D.n_nodes ? 2 : 0) | (D.A.replica[u] ? 4 : 0);   // bit 2: border replica outside block 0 (not counted in norms)
    obs_unk.clear(); unk_obs.assign(D.A.n_unk, -1);
    obs_primary.clear();
    for (size_t o = 0; o < D.obs_kind.size(); ++o) {
      int u = -1;
      if (D.obs_kind[o] == 0) u = D.A.node_unknown[D.obs_index[o]];
      else { int b = D.dev[D.obs_index[o]].branch; u = b >= 0 ? D.A.branch_unknown[b] : -1; }
      obs_unk.push_back(u);
      int prim = (int)o;
      if (u >= 0) { if (unk_obs[u] < 0) unk_obs[u] = (int)o; else prim = unk_obs[u]; }
      obs_primary.push_back(prim);
    }
  }
  void size_lds(const Description& D) {
    lds_doubles_fixed = 0; lds_extra_bytes = 0; lds_plan_bytes = 0; lds_pad_doubles = 0;
    for (size_t ci = 0; ci < D.A.classes.size(); ++ci) {
      const CompClass& c = D.A.classes[ci];
      lds_doubles_fixed = std::max(lds_doubles_fixed, (size_t)c.ndev * D.A.stride() + (size_t)c.nc * (c.nc + 1) + (size_t)c.nc * c.nc + 12 * (size_t)c.nc);
      lds_extra_bytes = std::max(lds_extra_bytes, ((size_t)h_cms[ci].blob_ints + 64) * 4 + 16);  // blob + the block's MOS class list
      lds_plan_bytes = std::max(lds_plan_bytes, (size_t)h_cms[ci].spare0 * 4);     // the gather schedule behind the blob (device-resident stepper only)
      lds_pad_doubles = std::max(lds_pad_doubles, (size_t)GatherStrides::of(D.A.wide, D.A.nb, D.A.max_nc, c.nc).extra_doubles(c.nc));   // its padded images of A and C
    }
  }
};
// ---- sample tables: S and slot_val come from ch_set_samples / ch_set_params, the rest is rebuilt by finalize_params when dirty ----
// The ParamTables base is the host side (widths, tables, MOS classes, per-block class lists: ch_param_tables.hpp), kept as uploaded:
// the sensitivities copy from it, the source evaluation and the torn companion's border devices read it.
struct SampleTables : ParamTables {
  int S = 1; bool dirty = true;
  std::vector<std::vector<double>> slot_val;  // [n_slot][S] or empty
  long vac_stride_ = 0;
  DevBuf<double> d_dpar, d_dmult, d_gmin, d_temp, d_mosp, d_vapar, d_vacache;
  DevBuf<int> d_dcls, d_moscls_inst, d_mc_ofs, d_mc_n, d_mc_list, d_dcls_local;
  DevBuf<BlockMeta> d_bmeta;   // (holds each block's MOS class list, hence here and not in the structure)
};
// the source tables a source evaluation reads: the circuit's, or a perturbed copy of either
struct SourceTables { const std::vector<double>* dc; const std::vector<double>* par; };
// ---- Newton state: the rings, the launch scratch and the argument template; sized by finalize_params, written by every solve ----
struct NewtonState {
  DevBuf<double> d_X, d_Q, d_rate, d_kv;   // state and charge rings; d_kv = [kv | srcv] contiguous
  DevBuf<unsigned char> d_perm, d_active;  // pivot order of every block's register LU (NewtonArgs::perm); per-block active mask
  DevBuf<BlockOut> d_out; PinnedBuf<BlockOut> h_out;    // per-block records: device, or mapped pinned [n_comp*S]
  PinnedBuf<Summary> h_sum; PinnedBuf<double> h_stage;  // pinned: the summary; staging for kv/srcv uploads
  DevEvent ev0, ev1; bool host_reduce = true; size_t lds_bytes = 0;   // events of a timed launch; host_reduce: block outputs land in mapped host memory and the host reduces them
  int path = 1;                 // 1 = fused block kernel, 2 = sparse level-scheduled LU
  NewtonArgs base;              // structure pointers filled once
  mutable std::vector<double> all_src; std::vector<double> sv_buf, kv_buf;   // host scratch of eval_sources / set_sources
};
// ---- sparse path (blocks too large for LDS): ch_engine_sparse.hpp and the path == 2 branches ----
// grid sizes of the sparse path's kernels (x; y walks the sample list): gn rows / 256, gd devices / 64, ga max(rows, entries) / 256.
// The O(n) passes (norms, update, commit) run in one workgroup per sample for small systems and, from 4096 rows (`many`), in nbr <=
// SP_NP workgroups + a finishing pass.
struct SpGrids { int gn, gd, ga, nbr; bool many; };
struct SparsePath {
  SparsePlan plan[2];           // [0] DC (alpha0 = 0), [1] transient
  struct PlanDev { DevBuf<int> idx[SP_N_PLAN_ARRAYS];   // one buffer per row of SP_PLAN_ARRAYS (ch_sparse.hpp)
                   DevBuf<double> LUv, Lv;
                   DevBuf<int> s3_blob, s3_ptr, s3_topa, s3_topr; DevBuf<double> s3_schur, s3_xT, s3_base, s3_sum; DevBuf<unsigned> s3_cnt;
                   bool s3 = false; Sp3Dev s3_dev; unsigned s3_lds = 0; } plan_dev[2];   // subtree form in use: its kernel arguments and LDS bytes
  DevBuf<int> dflag; DevBuf<double> part;   // part: [S][8][SP_NP] per-workgroup partial reductions of the O(n) passes (ch_sparse.hpp)
  DevBuf<double> hpart, hrow;   // slices of the heavy assembly items [S][items][SP_HB][2] and of the heavy rows of the charge update [S][rows][SP_RB]
  DevBuf<int> rowptr, colidx, mat_gptr, mat_gsrc, vec_gptr, vec_gsrc, heavy_mat, heavy_vec, heavy_rows; int n_heavy_mat = 0, n_heavy_vec = 0, n_heavy_rows = 0;
  DevBuf<double> stage, Aval, Cval, F, Q, rhs, y, dx, xcur, xpred, hq, w, qn;
  std::vector<int> h_rowptr, h_colidx; PinnedBuf<double> h_red; PinnedBuf<int> h_flag;  // CSR pattern; mapped pinned: [S][8], [S][2]
  SparseNewton newton;          // the per-sample decisions of a solve; keeps rate_v / status_v between solves (ch_sparse_newton.hpp)
  SpGrids grid{};               // filled by build_sparse_structure
  DevBuf<int> act[3]; DevBuf<double> scale;   // device copies of a sample list / the per-sample scales (stage_list)
  PinnedBuf<int> h_act; PinnedBuf<double> h_scale;
};
// ---- device-resident step controller: ch_engine_persist.hpp ----
struct DeviceStepper {
  DevBuf<int> d_pci; DevBuf<double> d_pcd, d_pbps, d_psave, d_prows; DevBuf<TranCtl> d_pctl; DevBuf<int> d_pwgc, d_pwgk; DevBuf<double> d_pdcent, d_ptrans;
  // ONE allocation [times | point counts | workgroup records | group records | counters]: everything behind the times is cleared
  // by one memset per launch (persist_io_layout, ch_engine_persist.hpp)
  DevBuf<double> d_pio;
  // what the constant buffers hold (the launch's constants are the same from transient to transient on one circuit: they are
  // uploaded when they differ from this, or when their buffer is new)
  std::vector<int> h_pci, h_pwgc, h_pwgk; std::vector<double> h_pcd, h_pbps, h_psave;
  PinnedBuf<double> h_stage;    // pinned: constants on their way up, the controller state both ways, the read-back of a finished launch
  const void* attr_fn = nullptr; size_t attr_static_lds = 0;   // the kernel whose attributes were read and set last (once per function, not per call)
  int n_cu = 0, mode = 0; bool aborted = false;   // aborted: the last device-stepper launch gave up on a wait (its workgroups were not co-resident: another process's kernel held part of the GPU)
};
// host seconds of one transient by stage (CEDARHIP_HOST_PROFILE; printed by finish_tran)
struct HostLaps {
  double start_vector = 0, dc_copies = 0, dc_wait = 0, charges = 0, consts = 0, launch_sync = 0, readback = 0, collect = 0;
};
// the time since the last mark (or the construction) goes to the lap named; one branch when the profile is off
struct LapTimer {
  const bool on; hclock::time_point t;
  explicit LapTimer(bool on_) : on(on_), t(on_ ? hclock::now() : hclock::time_point()) {}
  void lap(double& acc) { if (on) { const auto n = hclock::now(); acc += std::chrono::duration<double>(n - t).count(); t = n; } }
};
// ---- small signal: ch_engine_ac.hpp (ch_eval shares the A / F / Q dumps) ----
// the source table of the last ch_noise_ex on the host (ch_noise_sources reads it): [S][n_tab] entries of block `comp`, and the
// MOSFET operand rows [S][ndev][B4NO_COUNT]
struct LastNoise {
  bool valid = false, mos = false; int comp = -1, S = 0, n_tab = 0, ndev = 0;
  std::vector<int> a, b; std::vector<double> pwr, ex, op;
};
struct SmallSignal {
  // MOSFET noise (ch_noise_ex): the noise rows ch_set_mos_noise gave, [model] empty or CH_B4N_NPAR; the per-class table, the operand
  // rows and the entry-to-column map of the contributions of one analysis
  std::vector<std::vector<double>> mos_noise_given; LastNoise last_noise;
  std::vector<double> mos_npar_host;   // the per-class table of the last analysis with MOSFET noise, as uploaded (ch_noise_sens adds a row to a copy)
  DevBuf<double> d_mos_npar, d_mos_op; DevBuf<int> d_mos_fail, d_contrib_col;
  DevBuf<double> d_dumpA, d_dumpF, d_dumpQ, d_dumpC, d_dumpG, d_dumpF0, d_omega, d_xac, d_psd, d_noise_pwr, d_noise_exp;
  DevBuf<int> d_noise_a, d_noise_b, d_acfail; DevBuf<BlockMeta> d_bmeta_all;
  double scale = 0.0;           // eval_sources adds scale*|ac| to every source value (AC right-hand side)
};
// ---- DC sensitivities: ch_engine_sens.hpp (the G / F dumps are SmallSignal's) ----
struct Sensitivity {
  DevBuf<double> d_Fp, d_Fm, d_den, d_x;                                          // F(p + h), F(p - h) or F(p) per parameter; divisors; results
  DevBuf<double> d_dpar, d_dmult, d_gmin, d_temp, d_mosp, d_vapar, d_vacache;     // device copies of what perturb_tables returns
  DevBuf<int> d_dcls, d_dcls_local, d_mc_list, d_skip, d_fail; DevBuf<BlockMeta> d_bmeta;
  // AC sensitivities (ch_ac_sens): ONE pair of dense G / C dumps per sign, reused by every parameter pass; the complex right-hand
  // sides [n_par][nblk][n_freq][ds][2]; divisors and state-term steps [n_par][S]; results [S][n_freq][n_par][n_unk][2]
  DevBuf<double> d_Gp, d_Gm, d_Cp, d_Cm, d_R, d_den_ac, d_eps, d_xac_sens;
};
// ---- noise sensitivities: ch_engine_noisesens.hpp (restricted to the output block; dumps, tables and steps are the two above's) ----
struct NoiseSensitivity {
  DevBuf<double> d_y, d_R, d_dpwr, d_dpsd;                       // [S][n_freq][nc][2]; [n_par][S][n_freq][ds][2]; [n_par][S][n_tab]; [S][n_freq][n_par]
  DevBuf<double> d_pwr_p, d_pwr_m, d_ex_p, d_ex_m, d_kv, d_npar; // source tables of the two signs, known-node values and MOSFET noise rows they are built with
  DevBuf<int> d_na, d_nb, d_ex_moved;                            // terminals of those tables (not read); [n_par] flags: a table's exponent differs
};
// ---- torn companion ----
// A coupled array behind a border of one or two unknowns (supply rails with a series resistance): the same description analysed
// with tearing (ch_analysis.hpp) — independent blocks + border replicas.  It only ever runs transients on the device-resident
// stepper, started from this circuit's (sparse-path) operating point; everything else stays on this circuit.
struct TornCompanion {
  std::unique_ptr<ch_circuit> c; std::string note;
  bool is_torn = false, keep_slot0 = false;
  std::vector<int> dsrc_host;               // per flattened device: source slot (or Verilog-A parameter offset), as uploaded
};

struct ch_circuit {
  Arena arena;  // declared first: destroyed last, after every DevBuf that points into it
  ch_ctx* ctx = nullptr;
  Description desc; Structure stru; SampleTables tab; NewtonState nwt;   // the groups above
  SparsePath sp; DeviceStepper ps; SmallSignal ac; Sensitivity sens; NoiseSensitivity nsens; TornCompanion torn; LaunchStats stats;   // (LaunchStats: ch_stepper_host.hpp)
  DcStart dc_start; DevBuf<double> d_dc_start;   // the first DC pass' start vector, drawn once per (seed, S): host side (ch_dc_start.hpp) and its device copy
  HostLaps laps;
  const bool host_profile = env_on(Env::HOST_PROFILE);
  const long time_every = std::max(1L, env_long(Env::TIME_EVERY, 8));  // device_ms sums the sampled launches only

  std::string& err() { return ctx->err; }
  void set_err(const std::string& s) { ctx->err = s; }

  ~ch_circuit() {
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);  // a polled launch may still be retiring
    if (g_arena == &arena) g_arena = nullptr;
  }

  // ------------------------------------------------------------------------------------------
  int upload_structure() {
    g_arena = &arena; hipStream_t st = ctx->stream;
    std::vector<int> blob, dkind, dterm, dhdev, dvac, vmod, vpofs, vcofs, obs_unk, unk_obs; std::vector<unsigned char> dm;
    std::vector<int>& dsrc = torn.dsrc_host;
    stru.class_blobs(desc, blob);
    stru.source_lists(desc, dkind, dterm, dhdev, dsrc);
    stru.va_offsets(desc, dvac, vmod, vpofs, vcofs);
    HIPCHK(stru.d_dvac.upload(dvac, st)); HIPCHK(stru.d_va_mod.upload(vmod, st)); HIPCHK(stru.d_va_pofs.upload(vpofs, st)); HIPCHK(stru.d_va_cofs.upload(vcofs, st));
    stru.masks_and_observables(desc, dm, obs_unk, unk_obs);
    HIPCHK(stru.d_unk_obs.upload(unk_obs, st));
    { std::vector<unsigned long long> z(8, 0ull); HIPCHK(stru.d_stamps.upload(z, st)); }
    HIPCHK(stru.d_classes.upload(stru.h_cms, st)); HIPCHK(stru.d_gl_ptr.upload(blob, st));
    HIPCHK(stru.d_comp_class.upload(desc.A.comp_class, st)); HIPCHK(stru.d_comp_uofs.upload(desc.A.comp_uofs, st)); HIPCHK(stru.d_comp_dofs.upload(desc.A.comp_dofs, st));
    HIPCHK(stru.d_dkind.upload(dkind, st)); HIPCHK(stru.d_dterm.upload(dterm, st)); HIPCHK(stru.d_dsrc.upload(dsrc, st)); HIPCHK(stru.d_dhdev.upload(dhdev, st));
    HIPCHK(stru.d_dmask.upload(dm, st)); HIPCHK(stru.d_obs_unk.upload(obs_unk, st));
    HIPCHK(nwt.h_sum.alloc(1, hipHostMallocMapped)); HIPCHK(nwt.ev0.create()); HIPCHK(nwt.ev1.create());
    stru.size_lds(desc);
    return CH_OK;
  }

  SlotValues slots() const { return SlotValues{desc, tab.slot_val, tab.S}; }
  double slot_value(int i, int s) const { return slots().value(i, s); }

  // bias-independent constants of every compiled Verilog-A instance from parameter blocks and temperatures (device pointers, in the
  // circuit's widths) -> dst, one block per sample when either varies; once per parameter / temperature change
  int launch_va_setup(const double* vapar, const double* temp, DevBuf<double>& dst) {
    const int Svac = (tab.Sva > 1 || tab.Stemp > 1) ? tab.S : 1;
    HIPCHK(dst.alloc(std::max<size_t>(1, stru.vac_total * (size_t)Svac)));
    if (stru.n_va_inst == 0) return CH_OK;
    const long nthr = (long)stru.n_va_inst * Svac;
    hipLaunchKernelGGL(va_setup_kernel, dim3((unsigned)((nthr + 63) / 64)), dim3(64), 0, ctx->stream, stru.n_va_inst, Svac, stru.d_va_mod.p, stru.d_va_pofs.p, stru.d_va_cofs.p,
                       vapar, tab.Sva > 1 ? (long)std::max<size_t>(1, desc.va_par.size()) : 0L, temp, tab.Stemp, dst.p, Svac > 1 ? (long)stru.vac_total : 0L);
    HIPCHK(hipGetLastError());
    return CH_OK;
  }

 private:   // ---- the steps of finalize_params, in its order ----
  // the state rings alone take 2 * NSLOT * S * n_unk doubles: refuse a sample count the device cannot hold before any
  // host table is sized by it (the caller gets an error code, not a std::bad_alloc or a half-built circuit)
  int check_capacity() {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const double need = 2.0 * NSLOT * (double)tab.S * (double)std::max(1, desc.A.n_unk) * sizeof(double) + 64.0 * (double)tab.S * (double)std::max(1, desc.A.n_comp);
    if (need > 0.9 * (double)total_b) { set_err("sample count does not fit the device: " + std::to_string(tab.S) + " samples of " + std::to_string(desc.A.n_unk) + " unknowns need " + std::to_string((long long)(need / 1048576.0)) + " MiB for the state rings"); return CH_ERR_NOMEM; }
    return CH_OK;
  }
  // the host tables (build_param_tables, ch_param_tables.hpp), their upload and the Verilog-A setup launch
  int upload_tables() {
    hipStream_t st = ctx->stream;
    const int rc = build_param_tables(desc, slots(), stru.h_cms, tab, err());
    if (rc != CH_OK) return rc;
    HIPCHK(tab.d_dpar.upload(tab.dpar, st)); HIPCHK(tab.d_dmult.upload(tab.dmult, st)); HIPCHK(tab.d_gmin.upload(tab.gmin, st)); HIPCHK(tab.d_temp.upload(tab.temp, st));
    HIPCHK(tab.d_vapar.upload(tab.vapar, st));
    HIPCHK(tab.d_mosp.upload(tab.mosp, st)); HIPCHK(tab.d_dcls.upload(tab.dcls, st));
    HIPCHK(tab.d_bmeta.upload(tab.bmeta, st));
    HIPCHK(tab.d_mc_ofs.upload(tab.mc_ofs, st)); HIPCHK(tab.d_mc_n.upload(tab.mc_n, st)); HIPCHK(tab.d_mc_list.upload(tab.mc_list, st)); HIPCHK(tab.d_dcls_local.upload(tab.dcls_local, st));
    HIPCHK(tab.d_moscls_inst.upload(tab.mos_cls, st));
    const int rcv = launch_va_setup(tab.d_vapar.p, tab.d_temp.p, tab.d_vacache);
    tab.vac_stride_ = (tab.Sva > 1 || tab.Stemp > 1) ? (long)stru.vac_total : 0L;
    if (host_profile) std::fprintf(stderr, "[tables] %zu bytes of host tables kept, %zu of them the packed MOSFET columns (%d classes x %d samples)\n", tab.retained_bytes(), tab.mosp.size() * sizeof(double), tab.n_cls, tab.Smos);
    return rcv;
  }
  // state ring and outputs
  int alloc_rings() {
    hipStream_t st = ctx->stream;
    const size_t slot_elems = (size_t)tab.S * desc.A.n_unk;
    HIPCHK(nwt.d_X.alloc(slot_elems * NSLOT)); HIPCHK(nwt.d_Q.alloc(slot_elems * NSLOT));
    HIPCHK(hipMemsetAsync(nwt.d_X.p, 0, slot_elems * NSLOT * sizeof(double), st));
    HIPCHK(hipMemsetAsync(nwt.d_Q.p, 0, slot_elems * NSLOT * sizeof(double), st));
    HIPCHK(nwt.d_out.alloc((size_t)desc.A.n_comp * tab.S));
    { std::vector<double> ones((size_t)desc.A.n_comp * tab.S, 1.0); HIPCHK(nwt.d_rate.upload(ones, st)); }
    HIPCHK(nwt.d_perm.alloc((size_t)desc.A.n_comp * tab.S * 16)); HIPCHK(hipMemsetAsync(nwt.d_perm.p, 0, (size_t)desc.A.n_comp * tab.S * 16, st));   // identity
    nwt.host_reduce = (size_t)desc.A.n_comp * tab.S <= 4096 && !env_on(Env::DEVICE_REDUCE);
    if (nwt.host_reduce && nwt.h_out.n < (size_t)desc.A.n_comp * tab.S) {
      HIPCHK(nwt.h_out.alloc((size_t)desc.A.n_comp * tab.S, hipHostMallocMapped));
      std::memset(nwt.h_out, 0, (size_t)desc.A.n_comp * tab.S * sizeof(BlockOut));   // sequence numbers start at 1
    }
    HIPCHK(nwt.d_active.alloc((size_t)desc.A.n_comp * tab.S));
    const size_t need = (size_t)tab.Ssrc * (desc.A.known.size() + stru.n_dev_src());
    HIPCHK(nwt.d_kv.alloc(need));  // [kv | srcv] contiguous: one upload per step
    if (need > nwt.h_stage.n) HIPCHK(nwt.h_stage.alloc(need));
    return CH_OK;
  }
  // argument template, LDS footprint and the path decision
  int fill_base() {
    const long cols = tab.mos_cols(); const size_t slot_elems = (size_t)tab.S * desc.A.n_unk;
    NewtonArgs& a = nwt.base;
    std::memset(&a, 0, sizeof(a));
    a.comp_class = stru.d_comp_class.p; a.comp_uofs = stru.d_comp_uofs.p; a.comp_dofs = stru.d_comp_dofs.p; a.classes = stru.d_classes.p;
    a.blob = stru.d_gl_ptr.p; a.dkind = stru.d_dkind.p; a.dterm = stru.d_dterm.p; a.dsrc = stru.d_dsrc.p; a.dcls = tab.d_dcls.p; a.dhdev = stru.d_dhdev.p;
    a.dpar = tab.d_dpar.p; a.dmult = tab.d_dmult.p; a.mosp = tab.d_mosp.p; a.mos_cols = cols; a.kv = nwt.d_kv.p; a.srcv = nwt.d_kv.p + (size_t)tab.Ssrc * desc.A.known.size(); a.dmask = stru.d_dmask.p;
    a.active = nullptr; a.gmin_s = tab.d_gmin.p; a.vapar = tab.d_vapar.p; a.va_stride = tab.Sva > 1 ? (long)std::max<size_t>(1, desc.va_par.size()) : 0; a.temp_s = tab.d_temp.p; a.Stemp = tab.Stemp;
    a.vacache = tab.d_vacache.p; a.vac_stride = tab.vac_stride_; a.dvac = stru.d_dvac.p;
    a.n_comp = desc.A.n_comp; a.S = tab.S; a.Spar = tab.Spar; a.Ssrc = tab.Ssrc; a.Smos = tab.Smos; a.Sgmin = tab.Sgmin; a.nk = (int)desc.A.known.size(); a.nsrc = stru.n_dev_src();
    a.n_unk = desc.A.n_unk; a.n_mos_cls = tab.n_cls;
    a.X = nwt.d_X.p; a.Qh = nwt.d_Q.p; a.slot_stride = (long)slot_elems; a.out = nwt.host_reduce ? nwt.h_out.p : nwt.d_out.p;
    a.unk_obs = stru.d_unk_obs.p; a.n_obs = (int)desc.obs_kind.size();
    a.bmeta = tab.d_bmeta.p; a.dcls_local = tab.d_dcls_local.p; a.comp_mc_ofs = tab.d_mc_ofs.p; a.comp_mc_n = tab.d_mc_n.p; a.mc_list = tab.d_mc_list.p; a.max_mc = tab.max_mc;
    a.summary = nwt.h_sum; a.rate = nwt.d_rate.p; a.perm = nwt.d_perm.p;
#ifdef CH_STAMPS
    a.stamps = stru.d_stamps.p;
#endif
    nwt.lds_bytes = (stru.lds_doubles_fixed + desc.A.known.size() + stru.n_dev_src() + (size_t)tab.max_mc * B4L_STRIDE) * sizeof(double) + stru.lds_extra_bytes;
    nwt.lds_bytes = std::max(nwt.lds_bytes, (size_t)9 * stru.block_threads * sizeof(double));  // scratch of the in-kernel reduction
    nwt.path = (nwt.lds_bytes > 150 * 1024 || desc.A.max_nc > 64 || tab.max_mc > 64 || desc.A.force_sparse || env_on(Env::FORCE_SPARSE)) ? 2 : 1;
    return CH_OK;
  }
 public:
  // ------------------------------------------------------------------------------------------
  // (Re)build all per-sample parameter tables: remake(prob, p = sim) for every sample at once.
  int finalize_params() {
    if (!tab.dirty) return CH_OK;
    g_arena = &arena;
    for (int (ch_circuit::*step)() : {&ch_circuit::check_capacity, &ch_circuit::upload_tables, &ch_circuit::alloc_rings, &ch_circuit::fill_base})
      { const int rc = (this->*step)(); if (rc != CH_OK) return rc; }
    if (nwt.path == 2) { const int rcs = build_sparse_structure(); if (rcs != CH_OK) return rcs; nwt.lds_bytes = 0; }
    // (the kernels' dynamic-LDS ceiling is raised once per device in ch_create: a per-circuit setting would be lowered again
    //  by the next, smaller circuit of the same process)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    tab.dirty = false;
    return CH_OK;
  }

  // host evaluation of source and known-node values for sample set s at time t, from the circuit's source tables or the given ones
  SourceTables own_sources() const { return SourceTables{&tab.src_dc, &tab.src_par}; }
  void eval_sources(double t, int mode, std::vector<double>& sv, std::vector<double>& kv) const { eval_sources(t, mode, sv, kv, own_sources()); }
  void eval_sources(double t, int mode, std::vector<double>& sv, std::vector<double>& kv, SourceTables src) const {
    const int nsrc = (int)desc.src.size(), nk = (int)desc.A.known.size(), nds = stru.n_dev_src();
    sv.assign((size_t)tab.Ssrc * nds, 0.0); kv.assign((size_t)tab.Ssrc * nk, 0.0);
    nwt.all_src.resize(std::max(1, nsrc));
    for (int s = 0; s < tab.Ssrc; ++s) {
      for (int i : stru.needed_src) nwt.all_src[i] = source_value(desc.src[i], &(*src.par)[((size_t)s * nsrc + i) * CH_SRC_NPAR], (*src.dc)[(size_t)s * nsrc + i], t, mode) + ac.scale * desc.src[i].ac;
      for (size_t j = 0; j < stru.dev_src.size(); ++j) sv[(size_t)s * nds + j] = nwt.all_src[stru.dev_src[j]];
      for (int k = 0; k < nk; ++k) { double v = 0; for (auto& tm : desc.A.known[k].terms) v += tm.second * nwt.all_src[tm.first]; kv[(size_t)s * nk + k] = v; }
    }
  }
  int set_sources(NewtonArgs& a, double t, int mode) { return set_sources(a, t, mode, own_sources()); }
  int set_sources(NewtonArgs& a, double t, int mode, SourceTables src) {
    std::vector<double>& sv = nwt.sv_buf; std::vector<double>& kv = nwt.kv_buf;
    eval_sources(t, mode, sv, kv, src);
    if (tab.Ssrc == 1 && kv.size() + sv.size() <= (size_t)KV_INLINE) {
      a.inline_vals = 1;
      for (size_t i = 0; i < kv.size(); ++i) a.vals_inline[i] = kv[i];
      for (size_t i = 0; i < sv.size(); ++i) a.vals_inline[kv.size() + i] = sv[i];
      return CH_OK;
    }
    a.inline_vals = 0;
    // the pinned staging buffer is reused every step: the stream sync at the end of each step protects it
    std::memcpy(nwt.h_stage, kv.data(), kv.size() * sizeof(double));
    std::memcpy(nwt.h_stage + kv.size(), sv.data(), sv.size() * sizeof(double));
    HIPCHK(hipMemcpyAsync(nwt.d_kv.p, nwt.h_stage, (kv.size() + sv.size()) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    return CH_OK;
  }

  // ---- sparse path: ch_engine_sparse.hpp ----
  int build_sparse_structure();
  SparseDev sparse_dev(int which, int sm = 0);
  int sparse_plan_from_current(int which, int sm = 0);
  int stage_list(int slot, const std::vector<int>& list);
  void sp_launch_residual(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count);
  void sp_launch_norms(const NewtonArgs& a, const SparseDev& d, int what, const int* list, size_t count);
  void sp_launch_lu_solve(int which, const SparseDev& d, const int* list, size_t count);
  void sp_launch_update(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count, const double* scale);
  void sp_launch_commit(const NewtonArgs& a, const SparseDev& d, const int* list, size_t count);
  int sp_factor_and_step(const NewtonArgs& a, int which, bool fresh, bool damp);
  int run_sparse(NewtonArgs a, const unsigned char* host_active, Summary& out);
  // ---- small-signal analyses: ch_engine_ac.hpp ----
  int ac_ncomp() const { return nwt.path == 2 ? 1 : desc.A.n_comp; }
  int ac_ds() const { return nwt.path == 2 ? desc.A.n_unk : desc.A.max_nc; }
  int ac_comp_of(int u) const { return nwt.path == 2 ? 0 : (int)(std::upper_bound(desc.A.comp_uofs.begin(), desc.A.comp_uofs.end(), u) - desc.A.comp_uofs.begin()) - 1; }
  int ac_uofs(int comp) const { return nwt.path == 2 ? 0 : desc.A.comp_uofs[comp]; }
  int ac_nc(int comp) const { return nwt.path == 2 ? desc.A.n_unk : desc.A.comp_nc[comp]; }
  int ac_dofs(int comp) const { return nwt.path == 2 ? 0 : desc.A.comp_dofs[comp]; }
  int ac_ndev(int comp) const { return nwt.path == 2 ? (int)desc.A.edev.size() : desc.A.comp_ndev[comp]; }
  const BlockMeta* ac_bmeta();

  // the host thread has nothing else to do: poll for completion instead of sleeping on an interrupt.
  // (Watching the block records in mapped memory for a per-launch sequence number instead of the stream signal was
  // tried: the system-scope release each block then needs costs ~28 us per launch; profiles/r01_notes.md.)
  int poll_stream(const char* what) {
    hipError_t q = hipErrorNotReady;
    for (int spin = 0; spin < 200000 && q == hipErrorNotReady; ++spin) q = hipStreamQuery(ctx->stream);
    if (q == hipErrorNotReady) q = hipStreamSynchronize(ctx->stream);
    if (q != hipSuccess) { set_err(std::string(what) + hipGetErrorString(q)); return CH_ERR_DEVICE; }
    return CH_OK;
  }
  // host_active: host copy of the per-block active mask given to the kernel (DC restart passes, ch_eval), or null;
  // lds_extra: dynamic LDS bytes on top of lds_bytes (a perturbed evaluation of ch_dc_sens that stages one more BSIM4 column)
  int run_newton(const NewtonArgs& a, const unsigned char* host_active, Summary& out, size_t lds_extra = 0) {
    if (nwt.path == 2) return run_sparse(a, host_active, out);
    hipStream_t st = ctx->stream;
    const int nblk = desc.A.n_comp * tab.S;
    // kernel duration from the dispatch's own start/stop events on one launch in CEDARHIP_TIME_EVERY (default 8; timing every
    // launch costs ~5 us of host time per step)
    // sampled pseudo-randomly (a fixed stride aliases with the accept/reject rhythm of the stepper and biased the mean by 9 %)
    const bool timed = time_every <= 1 || ((uint64_t)(stats.n_launch + 1) * 0x9E3779B97F4A7C15ull >> 33) % (uint64_t)time_every == 0;
    const auto tp0 = host_profile ? hclock::now() : hclock::time_point();
    // timed launches carry their start/stop events in the dispatch itself (hipExtLaunchKernelGGL): the elapsed time is the
    // kernel's own begin-to-end, the quantity rocprofv3 --kernel-trace reports
    hipEvent_t e0 = timed ? nwt.ev0.e : nullptr, e1 = timed ? nwt.ev1.e : nullptr;
    const dim3 g(nblk), b(stru.block_threads);
    // (the order of this list is the order of the instantiations in the device code: each is emitted where it is first named)
    static void (*const kernels[])(const NewtonArgs) = {newton_block_kernel<16, true>, newton_block_kernel<0, true>, newton_block_kernel<8>, newton_block_kernel<12>,
                                                        newton_block_kernel<16>, newton_block_kernel<32>, newton_block_kernel<0>};
    const int lu = stru.lu_variant, ki = desc.A.wide ? (lu == 16 ? 0 : 1) : lu == 8 ? 2 : lu == 12 ? 3 : lu == 16 ? 4 : lu == 32 ? 5 : 6;
    hipExtLaunchKernelGGL(kernels[ki], g, b, (uint32_t)(nwt.lds_bytes + lds_extra), st, e0, e1, 0, a);
    if (!nwt.host_reduce) hipLaunchKernelGGL(reduce_blocks_kernel, dim3(1), dim3(256), 9 * 256 * sizeof(double), st, a);
    const auto tp1 = host_profile ? hclock::now() : hclock::time_point();
    { const int prc = poll_stream("newton kernel: "); if (prc != CH_OK) return prc; }
    HIPCHK(hipGetLastError());
    const auto tp2 = host_profile ? hclock::now() : hclock::time_point();
    if (timed) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, nwt.ev0, nwt.ev1)); stats.device_ms += ms; stats.n_timed += 1; }
    stats.n_launch += 1;
    if (!nwt.host_reduce) out = *nwt.h_sum;
    else {
      // host-side reduction of the per-block records (same arithmetic as reduce_all_blocks)
      Summary r; std::memset(&r, 0, sizeof(r));
      for (int s = 0; s < tab.S; ++s) {
        double e2[3] = {0, 0, 0}; long nd = 0; int smx = 0;
        for (int k = 0; k < desc.A.n_comp; ++k) {
          const size_t b = (size_t)k * tab.S + s;
          if (host_active && !host_active[b]) continue;
          const BlockOut& o = nwt.h_out[b];
          e2[0] += o.e2k; e2[1] += o.e2km1; e2[2] += o.e2kp1; nd += o.ndiff;
          if (o.status != 0) ++r.n_fail;
          if (o.status == 2) ++r.n_singular;
          smx = std::max(smx, o.iters); r.sum_block_iters += o.iters; r.fnorm = std::max(r.fnorm, o.fnorm);
        }
        r.sum_iters += smx; r.max_iters = std::max(r.max_iters, smx);
        if (nd > 0) { r.errk = std::max(r.errk, a.ck * std::sqrt(e2[0] / nd)); r.errkm1 = std::max(r.errkm1, a.ckm1 * std::sqrt(e2[1] / nd)); r.errkp1 = std::max(r.errkp1, a.ckp1 * std::sqrt(e2[2] / nd)); }
      }
      out = r;
    }
    if (host_profile) {
      const auto tp3 = hclock::now();
      stats.prof_launch += std::chrono::duration<double>(tp1 - tp0).count(); stats.prof_wait += std::chrono::duration<double>(tp2 - tp1).count();
      stats.prof_reduce += std::chrono::duration<double>(tp3 - tp2).count();
    }
    return CH_OK;
  }

  // unknown-space state of slot -> MNA vectors [S][n_mna]
  int download_mna(int slot, double t, int mode, double* x_out) {
    std::vector<double> xs((size_t)tab.S * desc.A.n_unk);
    HIPCHK(hipMemcpy(xs.data(), nwt.d_X.p + (size_t)slot * tab.S * desc.A.n_unk, xs.size() * sizeof(double), hipMemcpyDeviceToHost));
    unknowns_to_mna(xs.data(), t, mode, x_out);
    return CH_OK;
  }
  // xs: a slot's unknowns [S][n_unk], already on the host
  void unknowns_to_mna(const double* xs, double t, int mode, double* x_out) const {
    std::vector<double> sv, kv; eval_sources(t, mode, sv, kv);
    const int nk = (int)desc.A.known.size();
    for (int s = 0; s < tab.S; ++s) {
      double* xo = x_out + (size_t)s * desc.A.n_mna;
      for (int n = 1; n <= desc.n_nodes; ++n) xo[n - 1] = desc.A.node_unknown[n] >= 0 ? xs[(size_t)s * desc.A.n_unk + desc.A.node_unknown[n]] : kv[(size_t)(tab.Ssrc > 1 ? s : 0) * nk + desc.A.node_known[n]];
      for (int b = 0; b < desc.A.n_branch; ++b) xo[desc.n_nodes + b] = desc.A.branch_unknown[b] >= 0 ? xs[(size_t)s * desc.A.n_unk + desc.A.branch_unknown[b]] : CH_NAN;
    }
  }
  int upload_from_mna(int slot, const double* x_mna) {
    std::vector<double> xs((size_t)tab.S * desc.A.n_unk);
    for (int s = 0; s < tab.S; ++s) for (int u = 0; u < desc.A.n_unk; ++u) xs[(size_t)s * desc.A.n_unk + u] = x_mna[(size_t)s * desc.A.n_mna + desc.A.unk_mna[u]];
    HIPCHK(hipMemcpy(nwt.d_X.p + (size_t)slot * tab.S * desc.A.n_unk, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice));
    return CH_OK;
  }

  // ---- DC operating point: ch_engine_dc.hpp (dc_solve and its steps, in its order) ----
  int dc_solve(const ch_dc_opts& o, int slot, std::vector<int>* status_out, ch_stats* stt);
  int dc_start_vector(const ch_dc_opts& o);
  int dc_guess(NewtonArgs& a, const ch_dc_opts& o, int slot, int r, bool homotopy, DcRestarts& P);
  int dc_pass(NewtonArgs& a, const unsigned char* active, bool homotopy, Summary& sm);
  int dc_harvest(DcRestarts& P);

  // ---- device-resident step controller and the torn form: ch_engine_persist.hpp ----
  bool persist_eligible(std::string& why, bool own_steps);
  int persist_bpw(long nblk) const;
  bool persist_own_steps(const ch_tran_opts& o) const;
  size_t persist_wave_doubles(bool wg_consts) const;
  bool persist_blob(const std::vector<int>& kn, const std::vector<int>& ds, std::vector<int>& bi, std::vector<double>& bd, std::vector<int>& need) const;
  size_t persist_va_arena(int bpw, size_t& lds) const;
  int persist_stage(size_t doubles);
  int persist_upload_consts(const PersistConsts& pc, const std::vector<double>& bpu, const std::vector<double>& sv, bool wg_consts);
  bool persist_consts(bool wg_consts, int n_wg, int bpw, const TranPlan& p, PersistConsts& pc);
  int persist_fill_args(const TranPlan& p, const ch_dc_opts* dcm, PersistLaunch& L);
  PersistStep persist_pick_kernel(PersistLaunch& L);
  PersistStep persist_prepare(const TranPlan& p, const ch_dc_opts* dcm, PersistLaunch& L);
  int persist_launch(PersistLaunch& L, const TranCtl& cs, int resume, hipError_t& refused);
  int persist_drain(const PersistLaunch& L, ch_result* R, int resume, PersistRun& out, LapTimer& lt);
  int persist_readback(ch_result& R, size_t nt, const PersistIo& io, PersistRun& out);
  PersistStep persist_run(PersistLaunch& L, const TranPlan& p, ch_result* R, PersistRun& out);
  int persist_collect(ch_result& R, const PersistRun& out, bool own_steps, hclock::time_point tstart);
  PersistStep tran_persistent(const TranPlan& p, ch_result& R, hclock::time_point tstart);
  int dc_border(const ch_dc_opts& o, long long* iters);
  int tran_torn(double t0, double t1, const ch_tran_opts& o, ch_result& R, bool& used);

  // ---- transient driver: ch_engine_tran.hpp (tran_solve and its steps, in its order) ----
  int tran_solve(double t0, double t1, const ch_tran_opts& o, ch_result& R);
  int check_tran_opts(double t0, double t1, const ch_tran_opts& o);
  void tran_reset(ch_result& R);
  int tran_start(TranPlan& p, ch_result& R, hclock::time_point tstart, double other_seconds = 0.0);
  int tran_initial_state(const ch_tran_opts& o, ch_result& R);
  int tran_charges_at_t0(double t0, const ch_tran_opts& o, ch_result& R);
  int try_device_stepper(const TranPlan& p, ch_result& R, hclock::time_point tstart, bool& done);
  int save_row(ch_result& R, RowStore& rows, double ts, const int* slots, const double* w, int nw);
  int host_stepper_run(const TranPlan& p, ch_result& R, StepControl& sc, RowStore& rows, int& status);
  void host_stepper_collect(ch_result& R, const RowStore& rows);
  int finish_tran(ch_result& R, int newest_slot, double t, int status, hclock::time_point tstart, const double* xs_final = nullptr);

  // ---- transient sensitivities: ch_engine_transens.hpp (the run in progress, or null; the host stepper's loop calls the two hooks) ----
  TranSens* tsens = nullptr;
  int transens_after_accept(const StepControl& sc, const ch_result& R);
  int transens_save_row(long row, const int* slots, const double* w, int nw);
};
// What every entry point on a circuit opens: the circuit's arena for the allocations inside, a clean error text, its device.
struct CallScope { ArenaScope arena; explicit CallScope(ch_circuit* c) : arena(&c->arena) { c->ctx->err.clear(); (void)hipSetDevice(c->ctx->device); } };

#include "ch_engine_sparse.hpp"
#include "ch_engine_dc.hpp"
#include "ch_engine_persist.hpp"
#include "ch_engine_tran.hpp"


// Exception barrier of the C-ABI (include/cedarhip.h: "they never throw").  Host-side containers sized by the caller's
// input (samples x unknowns, blocks x ds^2, ...) can throw std::bad_alloc / std::length_error; letting that unwind through
// ctypes, a C client or a Julia ccall would end the host process in std::terminate.  The message goes to ch_last_error without
// allocating when memory is the problem.
static void set_err_nothrow(ch_ctx* ctx, const char* what, const char* detail) noexcept {
  if (!ctx) return;
  try { ctx->err = what; if (detail && *detail) { ctx->err += ": "; ctx->err += detail; } }
  catch (...) { ctx->err.clear(); }   // clear() does not allocate
}
template <class F>
static int guard_rc(ch_ctx* ctx, F&& body) noexcept {
  try { return body(); }
  catch (const std::bad_alloc&) { set_err_nothrow(ctx, "out of host memory inside the engine call", ""); return CH_ERR_NOMEM; }
  catch (const std::length_error& e) { set_err_nothrow(ctx, "a host container would exceed its maximum size (sample count x circuit size too large)", e.what()); return CH_ERR_NOMEM; }
  catch (const std::exception& e) { set_err_nothrow(ctx, "internal error (C++ exception caught at the C-ABI)", e.what()); return CH_ERR_INTERNAL; }
  catch (...) { set_err_nothrow(ctx, "internal error (unknown C++ exception caught at the C-ABI)", ""); return CH_ERR_INTERNAL; }
}

// =============================================================================================
extern "C" {

void ch_dc_opts_default(ch_dc_opts* o) { std::memset(o, 0, sizeof(*o)); o->abstol = 1e-10; o->maxiters = 200; o->n_restarts = 10; o->seed = 10; o->tran_mode = 0; o->dv_max = 2.0; o->x0 = nullptr; }
void ch_sens_opts_default(ch_sens_opts* o) { std::memset(o, 0, sizeof(*o)); o->rel_step = SENS_REL_STEP; o->abs_step = nullptr; }
void ch_tran_opts_default(ch_tran_opts* o) { std::memset(o, 0, sizeof(*o)); o->abstol = 1e-6; o->reltol = 1e-3; o->max_order = 5; o->newton_maxiters = 10; ch_dc_opts_default(&o->dc); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the (process-global) kernel function, not of a launch: it is set
// once per device to the largest size the path decision admits (finalize_params: 150 KB; ac_block_kernel<64>, sens_block_kernel<64> and transens_step_kernel<64>: 2*96*97 doubles; acsens_solve_kernel<64>, noisesens_solve_kernel<64>, loopgain_solve_kernel<64> and netparams_solve_kernel<64>: those factors plus a panel, launch_acsens / launch_noisesens / launch_loopgain / launch_netparams),
// so circuits with different LDS footprints can live side by side in one process.
static hipError_t raise_lds_ceilings() {
  const void* fns[] = {(const void*)newton_block_kernel<8>, (const void*)newton_block_kernel<12>, (const void*)newton_block_kernel<16>,
                       (const void*)newton_block_kernel<32>, (const void*)newton_block_kernel<0>, (const void*)newton_block_kernel<16, true>,
                       (const void*)newton_block_kernel<0, true>, (const void*)ac_block_kernel<64>, (const void*)sens_block_kernel<64>,
                       (const void*)acsens_solve_kernel<64>, (const void*)transens_step_kernel<64>, (const void*)noisesens_solve_kernel<64>,
                       (const void*)loopgain_solve_kernel<64>, (const void*)netparams_solve_kernel<64>};
  for (const void* f : fns) {
    hipFuncAttributes fa;
    hipError_t e = hipFuncGetAttributes(&fa, f);
    if (e != hipSuccess) return e;
    const int cap = lds_dynamic_ceiling((int)fa.sharedSizeBytes);
    e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static ch_ctx* ch_create_impl(int device_id, char* err, size_t errlen) {
  auto fail = [&](const std::string& m) -> ch_ctx* { if (err && errlen) { std::snprintf(err, errlen, "%s", m.c_str()); } return nullptr; };
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(std::string("cedarhip needs a HIP device (gfx950); none available: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0"));
  if (device_id < 0 || device_id >= n) return fail("invalid device id");
  if ((e = hipSetDevice(device_id)) != hipSuccess) return fail(hipGetErrorString(e));
  if ((e = raise_lds_ceilings()) != hipSuccess) return fail(std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
  ch_ctx* c = new ch_ctx();
  c->device = device_id;
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) { delete c; return fail(hipGetErrorString(e)); }
  return c;
}
void ch_destroy(ch_ctx* c) { if (!c) return; if (c->stream) (void)hipStreamDestroy(c->stream); delete c; }
const char* ch_last_error(ch_ctx* c) { return c ? c->err.c_str() : "null context"; }

static ch_circuit* ch_circuit_build_impl(ch_ctx* ctx, const ch_desc* d, bool tear = false) {
  if (!ctx || !d) return nullptr;
  ctx->err.clear();
  (void)hipSetDevice(ctx->device);
  std::unique_ptr<ch_circuit> owner(new ch_circuit());   // released on every early return and on an exception
  ch_circuit* c = owner.get();
  c->ctx = ctx;
  ArenaScope arena_scope(&c->arena);
  c->desc.n_nodes = d->n_nodes; c->desc.temp = d->temp; c->desc.gmin = d->gmin; c->desc.scale = d->scale;
  for (int i = 0; i < d->n_src; ++i) {
    HSource s; s.kind = d->src_kind[i]; s.dc = d->src_dc[i];
    for (int k = 0; k < CH_SRC_NPAR; ++k) s.par[k] = d->src_par[i * CH_SRC_NPAR + k];
    if (d->src_pwl_ofs) for (int k = d->src_pwl_ofs[i]; k < d->src_pwl_ofs[i + 1]; ++k) { s.ts.push_back(d->pwl_t[k]); s.ys.push_back(d->pwl_y[k]); }
    s.ac = d->src_ac ? std::fabs(d->src_ac[i]) : 0.0;
    c->desc.src.push_back(s);
  }
  for (int i = 0; i < d->n_model; ++i) c->desc.model.emplace_back(d->model_par + (size_t)i * CH_B4_NPAR, d->model_par + (size_t)(i + 1) * CH_B4_NPAR);
  auto bad = [&](const char* m) -> ch_circuit* { ctx->err = m; return nullptr; };
  for (int i = 0; i < d->n_dev; ++i) {
    HDev v; v.kind = d->dev_kind[i]; v.branch = -1; v.eliminated = false;
    for (int k = 0; k < CH_DEV_NNODE; ++k) { v.node[k] = d->dev_node[i * CH_DEV_NNODE + k]; if (v.node[k] < 0 || v.node[k] > d->n_nodes) return bad("device node id out of range"); }
    for (int k = 0; k < CH_DEV_NIPAR; ++k) v.ipar[k] = d->dev_ipar[i * CH_DEV_NIPAR + k];
    for (int k = 0; k < CH_DEV_NPAR; ++k) v.par[k] = d->dev_par[i * CH_DEV_NPAR + k];
    v.mult = d->dev_mult[i];
    if (v.mult < 0) return bad("Cannot construct a ParallelInstances with non-positive multiplier");
    if ((v.kind == CH_DEV_V || v.kind == CH_DEV_I) && (v.ipar[0] < 0 || v.ipar[0] >= d->n_src)) return bad("source index out of range");
    if (v.kind == CH_DEV_MOS && (v.ipar[0] < 0 || v.ipar[0] >= d->n_model)) return bad("model index out of range");
    if (v.kind < CH_DEV_R || v.kind > CH_DEV_VA) return bad("unknown device kind");
    if (v.kind == CH_DEV_VA) {
      if (v.ipar[0] < 0 || v.ipar[0] >= va_gen::N_MODULES) return bad("Verilog-A module id out of range (is the module compiled into this library?)");
      const va_gen::ModuleInfo& mi = va_gen::MODULES[v.ipar[0]];
      if (v.ipar[1] < 0 || (int64_t)v.ipar[1] + 2 * mi.n_params > d->n_va_par || !d->va_par) return bad("Verilog-A parameter block out of range");
      v.va_nt = mi.n_nodes; v.va_qmask = mi.q_mask;
    }
    c->desc.dev.push_back(v);
  }
  if (d->va_par && d->n_va_par > 0) c->desc.va_par.assign(d->va_par, d->va_par + d->n_va_par);
  for (int i = 0; i < d->n_slot; ++i) { c->desc.slot_kind.push_back(d->slot_kind[i]); c->desc.slot_a.push_back(d->slot_a[i]); c->desc.slot_b.push_back(d->slot_b[i]); }
  for (int i = 0; i < d->n_obs; ++i) { c->desc.obs_kind.push_back(d->obs_kind[i]); c->desc.obs_index.push_back(d->obs_index[i]); }
  c->tab.slot_val.assign(c->desc.slot_kind.size(), {});
  std::vector<char> protect(c->desc.dev.size(), 0), swept(c->desc.src.size(), 0);
  for (size_t o = 0; o < c->desc.obs_kind.size(); ++o) if (c->desc.obs_kind[o] == 1) { if (c->desc.obs_index[o] < 0 || c->desc.obs_index[o] >= (int)c->desc.dev.size()) return bad("observable device index out of range"); protect[c->desc.obs_index[o]] = 1; }
  for (size_t i = 0; i < c->desc.slot_kind.size(); ++i) {
    const int k = c->desc.slot_kind[i], sa = c->desc.slot_a[i], sb = c->desc.slot_b[i];
    bool ok = true;
    switch (k) {
      case CH_SLOT_DEV_PAR: ok = sa >= 0 && sa < (int)c->desc.dev.size() && sb >= 0 && sb < CH_DEV_NPAR; break;
      case CH_SLOT_DEV_MULT: ok = sa >= 0 && sa < (int)c->desc.dev.size(); break;
      case CH_SLOT_MODEL_PAR: ok = sa >= 0 && sa < (int)c->desc.model.size() && sb >= 0 && sb < CH_B4_NPAR; break;
      case CH_SLOT_SRC_DC: ok = sa >= 0 && sa < (int)c->desc.src.size(); break;
      case CH_SLOT_SRC_PAR: ok = sa >= 0 && sa < (int)c->desc.src.size() && sb >= 0 && sb < CH_SRC_NPAR; break;
      case CH_SLOT_TEMP: case CH_SLOT_GMIN: break;
      case CH_SLOT_VA_PAR: ok = sa >= 0 && (size_t)sa < c->desc.va_par.size(); break;
      default: ok = false;
    }
    if (!ok) return bad("parameter slot refers to a device, model, source or field that does not exist");
    if (k == CH_SLOT_SRC_DC || k == CH_SLOT_SRC_PAR) swept[sa] = 1;
  }
  // an AC-driven voltage source keeps its node and branch unknowns: the small-signal excitation enters one linear row
  for (size_t i = 0; i < c->desc.dev.size(); ++i) if (c->desc.dev[i].kind == CH_DEV_V && c->desc.src[c->desc.dev[i].ipar[0]].ac != 0.0) { protect[i] = 1; swept[c->desc.dev[i].ipar[0]] = 1; }
  int rc = analyse(c->desc.n_nodes, c->desc.dev, c->desc.src, protect, swept, c->desc.A, tear);
  if (rc != CH_OK) { ctx->err = c->desc.A.err; return nullptr; }
  c->torn.is_torn = tear;
  rc = c->upload_structure();
  if (rc != CH_OK) return nullptr;
  if (!tear && c->desc.A.max_nc > 64 && !env_on(Env::NO_TEAR)) {
    // one large coupled block: try the bordered block-diagonal form (refused, with a reason, for most circuits)
    c->torn.c.reset(ch_circuit_build_impl(ctx, d, true));
    c->torn.note = c->torn.c ? "torn companion built" : ctx->err;
    ctx->err.clear();
  }
  return owner.release();
}
void ch_circuit_free(ch_circuit* c) { delete c; }

int ch_circuit_info(ch_circuit* c, ch_info* o) {
  if (!c || !o) return CH_ERR_INVALID;
  std::memset(o, 0, sizeof(*o));
  const Analysis& A = c->desc.A;
  o->n_nodes = c->desc.n_nodes; o->n_branches = A.n_branch; o->n_mna = A.n_mna; o->n_unknowns = A.n_unk; o->n_known = (int)A.known.size() - 1;
  o->n_alias = A.n_alias; o->n_components = A.n_comp; o->max_component = A.max_nc; o->n_classes = (int)A.classes.size();
  o->n_mos = (int)A.mos_hdev.size(); o->n_mos_classes = c->tab.n_cls; o->path = c->nwt.path; o->n_samples = c->tab.S;
  o->nnz_jac = (int64_t)c->sp.h_colidx.size(); o->nnz_lu = c->sp.plan[1].valid ? c->sp.plan[1].nnz_lu : (c->sp.plan[0].valid ? c->sp.plan[0].nnz_lu : 0);
  return CH_OK;
}
// maps for tests / host mirrors: MNA index -> unknown (or -1) for nodes 0..n_nodes and branches
int ch_circuit_maps(ch_circuit* c, int32_t* node_unknown, int32_t* node_known, int32_t* branch_unknown) {
  if (!c) return CH_ERR_INVALID;
  for (int n = 0; n <= c->desc.n_nodes; ++n) { if (node_unknown) node_unknown[n] = c->desc.A.node_unknown[n]; if (node_known) node_known[n] = c->desc.A.node_known[n]; }
  for (int b = 0; b < c->desc.A.n_branch; ++b) if (branch_unknown) branch_unknown[b] = c->desc.A.branch_unknown[b];
  return CH_OK;
}

static int ch_set_samples_impl(ch_circuit* c, int32_t n) {
  if (!c) return CH_ERR_INVALID;
  if (n < 1) { c->set_err("ch_set_samples: at least one sample"); return CH_ERR_INVALID; }
  c->tab.S = n;
  for (auto& v : c->tab.slot_val) v.clear();
  c->tab.dirty = true;
  if (c->torn.c) return ch_set_samples_impl(c->torn.c.get(), n);
  return CH_OK;
}
static int ch_set_params_impl(ch_circuit* c, int32_t lo, int32_t hi, int32_t n_slots, const int32_t* ids, const double* values) {
  if (!c) return CH_ERR_INVALID;
  if (lo < 0 || hi > c->tab.S || lo >= hi || n_slots < 0 || (n_slots > 0 && (!ids || !values))) { c->set_err("ch_set_params: sample range outside [0, n_samples) or missing arrays"); return CH_ERR_INVALID; }
  for (int i = 0; i < n_slots; ++i) {
    const int id = ids[i];
    if (id < 0 || id >= (int)c->desc.slot_kind.size()) { c->set_err("slot id out of range"); return CH_ERR_INVALID; }
    auto& v = c->tab.slot_val[id];
    if (v.empty()) v.assign(c->tab.S, slot_base(c->desc, id));   // initialise with the description's base value
    for (int s = lo; s < hi; ++s) v[s] = values[(size_t)i * (hi - lo) + (s - lo)];
  }
  c->tab.dirty = true;
  if (c->torn.c) return ch_set_params_impl(c->torn.c.get(), lo, hi, n_slots, ids, values);
  return CH_OK;
}

static int ch_dc_impl(ch_circuit* c, const ch_dc_opts* o, double* x_out, int32_t* status_out, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  auto t0 = hclock::now();
  ch_stats st; std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  std::vector<int> status;
  rc = c->dc_solve(*o, 0, &status, &st);
  if (x_out) { int r2 = c->download_mna(0, 0.0, o->tran_mode ? 2 : 0, x_out); if (r2 != CH_OK) return r2; }
  if (status_out) for (int s = 0; s < c->tab.S; ++s) status_out[s] = status.empty() ? rc : status[s];
  st.wall_seconds = st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  c->stats.end_of_dc(st.n_block_iters); c->stats.fill(st); st.n_kernel_launches = c->stats.n_launch;
  if (stats) *stats = st;
  return rc;
}

static int ch_tran_impl(ch_circuit* c, double t0, double t1, const ch_tran_opts* o, ch_result** out) {
  if (!c || !o || !out) return CH_ERR_INVALID;
  CallScope call(c);
  std::unique_ptr<ch_result> R(new ch_result());
  R->ctx = c->ctx;
  int rc = c->tran_solve(t0, t1, *o, *R);
  R->status = rc;
  *out = R.release();
  return rc;
}
int64_t ch_result_n_times(const ch_result* r) { return r ? (int64_t)r->times.size() : 0; }
const double* ch_result_times(const ch_result* r) { return r ? r->times.data() : nullptr; }
const int32_t* ch_result_dense_points(const ch_result* r) { return (r && r->pts.size() == r->times.size()) ? r->pts.data() : nullptr; }
int ch_result_device_values(const ch_result* r, const double** ptr, int64_t* n_doubles) {
  if (!r || !ptr || !n_doubles) return CH_ERR_INVALID;
  *ptr = r->dev_values; *n_doubles = r->dev_n;
  return r->dev_values ? CH_OK : CH_ERR_UNSUPPORTED;
}
const double* ch_result_values(const ch_result* r) { return r ? r->values.data() : nullptr; }
const double* ch_result_final_state(const ch_result* r) { return r ? r->final_state.data() : nullptr; }
int ch_result_stats(const ch_result* r, ch_stats* s) { if (!r || !s) return CH_ERR_INVALID; *s = r->stats; return CH_OK; }
int ch_result_status(const ch_result* r) { return r ? r->status : CH_ERR_INVALID; }
void ch_result_free(ch_result* r) { delete r; }

static int ch_eval_impl(ch_circuit* c, int32_t sample, const double* x_mna, double t, double alpha0, int32_t mode, double* F_out, double* Q_out, double* J_out) {
  if (!c || !x_mna || sample < 0 || sample >= c->tab.S) return CH_ERR_INVALID;
  CallScope call(c);
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, nblk = A.n_comp * S, ds = A.max_nc;
  // state: only the requested sample matters
  std::vector<double> xs((size_t)S * A.n_unk, 0.0);
  for (int u = 0; u < A.n_unk; ++u) xs[(size_t)sample * A.n_unk + u] = x_mna[A.unk_mna[u]];
  if (hipMemcpy(c->nwt.d_X.p, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return CH_ERR_DEVICE;
  std::vector<unsigned char> act(nblk, 0);
  for (int k = 0; k < A.n_comp; ++k) act[(size_t)k * S + sample] = 1;
  if (hipMemcpy(c->nwt.d_active.p, act.data(), nblk, hipMemcpyHostToDevice) != hipSuccess) return CH_ERR_DEVICE;
  if (c->ac.d_dumpA.alloc((size_t)nblk * ds * ds) != hipSuccess || c->ac.d_dumpF.alloc((size_t)nblk * ds) != hipSuccess || c->ac.d_dumpQ.alloc((size_t)nblk * ds) != hipSuccess) return CH_ERR_DEVICE;
  NewtonArgs a = c->nwt.base;
  rc = c->set_sources(a, t, mode == 0 ? 0 : 1);
  if (rc != CH_OK) return rc;
  a.mode = MODE_EVAL; a.maxit = 1; a.alpha[0] = alpha0; a.hist_slot[0] = 0; a.cand_slot = 1; a.active = c->nwt.d_active.p; a.abstol = 1e-6; a.reltol = 1e-3;
  a.dumpA = c->ac.d_dumpA.p; a.dumpF = c->ac.d_dumpF.p; a.dumpQ = c->ac.d_dumpQ.p; a.dumpC = nullptr; a.dump_stride = ds;
  Summary sm;
  rc = c->run_newton(a, act.data(), sm);
  if (rc != CH_OK) return rc;
  const int n = A.n_mna;
  std::vector<char> has(n, 0);
  if (J_out) std::fill(J_out, J_out + (size_t)n * n, 0.0);
  if (F_out) std::fill(F_out, F_out + n, 0.0);
  if (Q_out) std::fill(Q_out, Q_out + n, 0.0);
  if (c->nwt.path == 2) {
    const size_t nnz = c->sp.h_colidx.size();
    std::vector<double> av(nnz), fv(A.n_unk), qv(A.n_unk);
    (void)hipMemcpy(av.data(), c->sp.Aval.p + (size_t)sample * nnz, nnz * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(fv.data(), c->sp.F.p + (size_t)sample * A.n_unk, fv.size() * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(qv.data(), c->sp.Q.p + (size_t)sample * A.n_unk, qv.size() * sizeof(double), hipMemcpyDeviceToHost);
    for (int u = 0; u < A.n_unk; ++u) {
      const int ri = A.unk_mna[u]; has[ri] = 1;
      if (F_out) F_out[ri] = fv[u];
      if (Q_out) Q_out[ri] = qv[u];
      if (J_out) for (int p = c->sp.h_rowptr[u]; p < c->sp.h_rowptr[u + 1]; ++p) J_out[(size_t)ri * n + A.unk_mna[c->sp.h_colidx[p]]] = av[p];
    }
  } else {
  std::vector<double> hA((size_t)nblk * ds * ds), hF((size_t)nblk * ds), hQ((size_t)nblk * ds);
  (void)hipMemcpy(hA.data(), c->ac.d_dumpA.p, hA.size() * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipMemcpy(hF.data(), c->ac.d_dumpF.p, hF.size() * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipMemcpy(hQ.data(), c->ac.d_dumpQ.p, hQ.size() * sizeof(double), hipMemcpyDeviceToHost);
  for (int k = 0; k < A.n_comp; ++k) {
    const int blk = k * S + sample, nc = A.comp_nc[k], uo = A.comp_uofs[k];
    for (int i = 0; i < nc; ++i) {
      const int ri = A.unk_mna[uo + i];
      has[ri] = 1;
      if (F_out) F_out[ri] = hF[(size_t)blk * ds + i];
      if (Q_out) Q_out[ri] = hQ[(size_t)blk * ds + i];
      if (J_out) for (int j = 0; j < nc; ++j) J_out[(size_t)ri * n + A.unk_mna[uo + j]] = hA[(size_t)blk * ds * ds + (size_t)i * nc + j];
    }
  }
  }
  if (J_out) for (int i = 0; i < n; ++i) if (!has[i]) J_out[(size_t)i * n + i] = 1.0;
  return CH_OK;
}

#include "ch_engine_ac.hpp"
#include "ch_engine_sens.hpp"
#include "ch_engine_noisesens.hpp"
#include "ch_engine_transens.hpp"
#include "ch_engine_measure.hpp"
#include "ch_engine_fmeasure.hpp"
#include "ch_engine_loopgain.hpp"
#include "ch_engine_netparams.hpp"


static int mos_eval_impl(ch_circuit* c, int32_t sample, const double* v, double* out, bool quad) {
  if (!c || !v || !out || sample < 0 || sample >= c->tab.S) return CH_ERR_INVALID;
  CallScope call(c);
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  const int nm = (int)c->desc.A.mos_hdev.size();
  if (nm == 0) return CH_OK;
  double *dv = nullptr, *dout = nullptr;
  if (hipMalloc((void**)&dv, (size_t)nm * 4 * sizeof(double)) != hipSuccess || hipMalloc((void**)&dout, (size_t)nm * 40 * sizeof(double)) != hipSuccess) return CH_ERR_DEVICE;
  (void)hipMemcpy(dv, v, (size_t)nm * 4 * sizeof(double), hipMemcpyHostToDevice);
  const double gm = c->tab.gmin[c->tab.Sgmin > 1 ? sample : 0];
  hipLaunchKernelGGL(quad ? mos_eval_quad_kernel : mos_eval_kernel, dim3(((quad ? 4 : 1) * nm + 63) / 64), dim3(64), 0, c->ctx->stream, (const double*)c->tab.d_mosp.p, c->nwt.base.mos_cols, (const int*)c->tab.d_moscls_inst.p, c->tab.Smos, (int)sample, nm, (const double*)dv, gm, dout);
  hipError_t e = hipStreamSynchronize(c->ctx->stream);
  if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)nm * 40 * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(dv); (void)hipFree(dout);
  if (e != hipSuccess) { c->set_err(hipGetErrorString(e)); return CH_ERR_DEVICE; }
  return CH_OK;
}
int ch_mos_eval(ch_circuit* c, int32_t sample, const double* v, double* out) { return guard_rc(c ? c->ctx : nullptr, [&] { return mos_eval_impl(c, sample, v, out, false); }); }
int ch_mos_eval_quad(ch_circuit* c, int32_t sample, const double* v, double* out) { return guard_rc(c ? c->ctx : nullptr, [&] { return mos_eval_impl(c, sample, v, out, true); }); }

static const char* const k_b4_names[] = {
#define P(n, d) #n,
#define B(n, d) #n, "l" #n, "w" #n, "p" #n,
#define I(n)
#include "../../include/cedarhip_bsim4_params.def"
};
static const char* const k_b4_ignored[] = {
#define P(n, d)
#define B(n, d)
#define I(n) #n,
#include "../../include/cedarhip_bsim4_params.def"
    nullptr};
int32_t ch_bsim4_npar(void) { return CH_B4_NPAR; }
const char* ch_bsim4_param_name(int32_t i) { return (i >= 0 && i < CH_B4_NPAR) ? k_b4_names[i] : nullptr; }
int32_t ch_bsim4_param_ignored(const char* name) {
  if (!name) return 0;
  for (int i = 0; k_b4_ignored[i]; ++i) if (std::strcmp(k_b4_ignored[i], name) == 0) return 1;
  return 0;
}
#include "ch_engine_diag.hpp"
int32_t ch_va_n_modules(void) { return va_gen::N_MODULES; }
int32_t ch_va_find(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < va_gen::N_MODULES; ++i) if (std::strcmp(va_gen::MODULES[i].name, name) == 0) return i;
  return -1;
}
const char* ch_va_module_name(int32_t id) { return (id >= 0 && id < va_gen::N_MODULES) ? va_gen::MODULES[id].name : nullptr; }
int32_t ch_va_module_info(int32_t id, int32_t* n_ports, int32_t* n_nodes, int32_t* n_params) {
  if (id < 0 || id >= va_gen::N_MODULES) return CH_ERR_INVALID;
  const va_gen::ModuleInfo& mi = va_gen::MODULES[id];
  if (n_ports) *n_ports = mi.n_ports; if (n_nodes) *n_nodes = mi.n_nodes; if (n_params) *n_params = mi.n_params;
  return CH_OK;
}
const char* ch_va_node_name(int32_t id, int32_t k) { return (id >= 0 && id < va_gen::N_MODULES && k >= 0 && k < va_gen::MODULES[id].n_nodes) ? va_gen::MODULES[id].node_names[k] : nullptr; }
const char* ch_va_param_name(int32_t id, int32_t k) { return (id >= 0 && id < va_gen::N_MODULES && k >= 0 && k < va_gen::MODULES[id].n_params) ? va_gen::MODULES[id].param_names[k] : nullptr; }
int32_t ch_va_n_opvars(int32_t id) { return (id >= 0 && id < va_gen::N_MODULES) ? va_gen::N_OPVARS[id] : 0; }
const char* ch_va_opvar_name(int32_t id, int32_t k) { return (id >= 0 && id < va_gen::N_MODULES && k >= 0 && k < va_gen::N_OPVARS[id]) ? va_gen::OPNAMES[id][k] : nullptr; }
// ---- the exported entry points: every body that can allocate runs behind an exception barrier ----
ch_ctx* ch_create(int device_id, char* err, size_t errlen) {
  try { return ch_create_impl(device_id, err, errlen); }
  catch (const std::exception& e) { if (err && errlen) std::snprintf(err, errlen, "ch_create: %s", e.what()); }
  catch (...) { if (err && errlen) std::snprintf(err, errlen, "ch_create: unknown C++ exception"); }
  return nullptr;
}
ch_circuit* ch_circuit_build(ch_ctx* ctx, const ch_desc* d) {
  ch_circuit* c = nullptr;
  const int rc = guard_rc(ctx, [&] { c = ch_circuit_build_impl(ctx, d); return c ? CH_OK : CH_ERR_INVALID; });
  return rc == CH_OK ? c : nullptr;   // on an exception the partially built circuit was already released by its owner (see ch_circuit_build_impl)
}
int ch_set_samples(ch_circuit* c, int32_t n) { return guard_rc(c ? c->ctx : nullptr, [&] { return ch_set_samples_impl(c, n); }); }
int ch_set_params(ch_circuit* c, int32_t lo, int32_t hi, int32_t n_slots, const int32_t* ids, const double* values) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_set_params_impl(c, lo, hi, n_slots, ids, values); });
}
int ch_dc(ch_circuit* c, const ch_dc_opts* o, double* x_out, int32_t* status_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_dc_impl(c, o, x_out, status_out, stats); });
}
int ch_tran(ch_circuit* c, double t0, double t1, const ch_tran_opts* o, ch_result** out) {
  if (out) *out = nullptr;
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_tran_impl(c, t0, t1, o, out); });
}
int ch_eval(ch_circuit* c, int32_t sample, const double* x_mna, double t, double alpha0, int32_t mode, double* F_out, double* Q_out, double* J_out) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_eval_impl(c, sample, x_mna, t, alpha0, mode, F_out, Q_out, J_out); });
}
int ch_ac(ch_circuit* c, const ch_dc_opts* o, int32_t n_freq, const double* freqs_hz, double* x_ac_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_ac_impl(c, o, n_freq, freqs_hz, x_ac_out, stats); });
}
int ch_noise(ch_circuit* c, const ch_dc_opts* o, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_noise_impl(c, o, out_kind, out_index, n_freq, freqs_hz, psd_out, stats); });
}
int ch_set_mos_noise(ch_circuit* c, int32_t model, const double* par) { return guard_rc(c ? c->ctx : nullptr, [&] { return ch_set_mos_noise_impl(c, model, par); }); }
int ch_noise_ex(ch_circuit* c, const ch_dc_opts* o, const ch_noise_opts* no, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out,
                double* contrib_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_noise_ex_impl(c, o, no, out_kind, out_index, n_freq, freqs_hz, psd_out, contrib_out, stats); });
}
int ch_noise_sources(ch_circuit* c, int32_t out_kind, int32_t out_index, int32_t sample, int32_t* n_src, int32_t* dev, int32_t* a, int32_t* b, double* pwr, double* ex,
                     double* mos_operands) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_noise_sources_impl(c, out_kind, out_index, sample, n_src, dev, a, b, pwr, ex, mos_operands); });
}
int ch_dc_sens(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, double* x_out, double* sens_out, int32_t* status_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_dc_sens_impl(c, o, n_par, slot_ids, so, x_out, sens_out, status_out, stats); });
}
int ch_ac_sens(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz,
               double* x_ac_out, double* dc_sens_out, double* sens_out, int32_t* status_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_ac_sens_impl(c, o, n_par, slot_ids, so, n_freq, freqs_hz, x_ac_out, dc_sens_out, sens_out, status_out, stats); });
}
int ch_noise_sens(ch_circuit* c, const ch_dc_opts* o, const ch_noise_opts* no, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t out_kind, int32_t out_index,
                  int32_t n_freq, const double* freqs_hz, double* psd_out, double* dpsd_out, double* dc_sens_out, int32_t* status_out, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_noise_sens_impl(c, o, no, n_par, slot_ids, so, out_kind, out_index, n_freq, freqs_hz, psd_out, dpsd_out, dc_sens_out, status_out, stats); });
}
int ch_tran_sens(ch_circuit* c, double t0, double t1, const ch_tran_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, ch_result** out) {
  if (out) *out = nullptr;
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_tran_sens_impl(c, t0, t1, o, n_par, slot_ids, so, out); });
}
int32_t ch_result_n_par(const ch_result* r) { return r ? r->n_par : 0; }
const double* ch_result_sens(const ch_result* r) { return (r && r->n_par > 0) ? r->sens.data() : nullptr; }
int ch_measure_rows(ch_ctx* ctx, int64_t n_times, const double* times, const int32_t* dense_points, int32_t n_rows, int32_t n_samples, const double* values, int32_t n_par,
                    const double* sens, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  return guard_rc(ctx, [&] { return ch_measure_rows_impl(ctx, n_times, times, dense_points, n_rows, n_samples, values, n_par, sens, n_meas, specs, out_value, out_sens, out_status); });
}
int ch_result_measure(const ch_result* r, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  if (!r || !r->ctx) return CH_ERR_INVALID;
  return guard_rc(r->ctx, [&] { return ch_result_measure_impl(r, n_meas, specs, out_value, out_sens, out_status); });
}
int ch_freq_measure_rows(ch_ctx* ctx, int32_t n_freq, const double* freqs_hz, int32_t n_rows, int32_t n_samples, const double* values, int32_t n_par, const double* sens,
                         int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status) {
  return guard_rc(ctx, [&] { return ch_freq_measure_rows_impl(ctx, n_freq, freqs_hz, n_rows, n_samples, values, n_par, sens, n_meas, specs, out_value, out_sens, out_status); });
}
int ch_ac_measure(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz, int32_t n_meas,
                  const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] { return ch_ac_measure_impl(c, o, n_par, slot_ids, so, n_freq, freqs_hz, n_meas, specs, out_value, out_sens, out_status, sample_status, stats); });
}
int ch_loop_gain(ch_circuit* c, const ch_dc_opts* o, int32_t probe_dev, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, int32_t n_freq, const double* freqs_hz,
                 double* T_out, double* dT_out, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status,
                 ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] {
    return ch_loop_gain_impl(c, o, probe_dev, n_par, slot_ids, so, n_freq, freqs_hz, T_out, dT_out, n_meas, specs, out_value, out_sens, out_status, sample_status, stats);
  });
}
int ch_net_params(ch_circuit* c, const ch_dc_opts* o, int32_t n_ports, const int32_t* port_devs, const double* z0, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so,
                  int32_t n_freq, const double* freqs_hz, double* S_out, double* Y_out, double* Z_out, double* dS_out, double* dY_out, double* dZ_out, int32_t n_meas,
                  const ch_fmeasure_spec* specs, double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats) {
  return guard_rc(c ? c->ctx : nullptr, [&] {
    return ch_net_params_impl(c, o, n_ports, port_devs, z0, n_par, slot_ids, so, n_freq, freqs_hz, S_out, Y_out, Z_out, dS_out, dY_out, dZ_out, n_meas, specs, out_value, out_sens,
                              out_status, sample_status, stats);
  });
}
int ch_bench_triad(ch_ctx* ctx, int64_t n, int32_t iters, double* gbps_out) { return guard_rc(ctx, [&] { return ch_bench_triad_impl(ctx, n, iters, gbps_out); }); }
int ch_bench_fp64(ch_ctx* ctx, int32_t iters, double* tflops_out) { return guard_rc(ctx, [&] { return ch_bench_fp64_impl(ctx, iters, tflops_out); }); }
int ch_debug_poison_lds(ch_ctx* ctx) { return guard_rc(ctx, [&] { return ch_debug_poison_lds_impl(ctx); }); }
int ch_debug_math(ch_ctx* ctx, int32_t which, int32_t n, const double* x, double* y) { return guard_rc(ctx, [&] { return ch_debug_math_impl(ctx, which, n, x, y); }); }
int ch_va_eval(ch_ctx* ctx, int32_t id, const double* par, const double* v, double temperature_k, double gmin, double* st_out) {
  return guard_rc(ctx, [&] { return ch_va_eval_impl(ctx, id, par, v, temperature_k, gmin, st_out); });
}
int ch_va_opvars(ch_ctx* ctx, int32_t id, const double* par, const double* v, double temperature_k, double gmin, double* op_out) {
  return guard_rc(ctx, [&] { return ch_va_opvars_impl(ctx, id, par, v, temperature_k, gmin, op_out); });
}
const char* ch_version(void) { return "cedarhip 0.3 (gfx950; fused block Newton, device-resident step controller)"; }

}  // extern "C"
