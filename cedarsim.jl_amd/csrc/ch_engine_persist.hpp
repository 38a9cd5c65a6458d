// ch_engine_persist.hpp — host side of the device-resident step controller (kernel: ch_persist.hpp): which circuits qualify,
// the constants blob, the launch and drain loop, and the torn form that only ever runs there.  Member functions of ch_circuit
// that own its DeviceStepper group (ps) and drive the TornCompanion (torn); included by ch_engine.hip behind the definition of ch_circuit.
#pragma once

// ------------------------------------------------------------------------------------------
// Device-resident step controller: which circuits qualify (ch_persist.hpp header), and the launch.
// Limits of the kernel's per-attempt source evaluation, checked by persist_eligible for the whole circuit and by persist_blob for
// every blob actually built: P_MAXSRC sources (one lane each), this many known-node + device-source values, this many PWL points.
constexpr size_t P_MAX_ENTRIES = 64, P_MAX_PWL = 2048;
// `own_steps`: the batch would run with per-sample step acceptance (no grid-wide wait anywhere in the kernel), so the workgroups
// need not be co-resident and any number of samples can be queued behind each other
inline bool ch_circuit::persist_eligible(std::string& why, bool own_steps) {
  auto no = [&](const char* m) { why = m; return false; };
  if (nwt.path != 1) return no("the circuit takes the sparse path");
  if (desc.A.n_comp < 1) return no("the circuit has no unknowns");
  if (!(stru.lu_variant == 8 || stru.lu_variant == 12 || stru.lu_variant == 16)) return no("a Jacobian block has more than 16 unknowns");
  if (desc.A.wide) {
    // compiled Verilog-A devices: every block of ONE class; a class with split (large) devices needs both halves of two blocks in
    // one wavefront each (wave pairs), any other class all its slots in one wavefront
    if (desc.A.classes.size() != 1) return no("compiled Verilog-A devices in blocks of several classes");
    if (desc.A.nb > 0) return no("compiled Verilog-A devices in a bordered form");
    if (stru.wide_split ? (stru.wide_l + stru.wide_other > 32) : (stru.h_cms[0].nslots > 64)) return no("a block's compiled devices need more evaluation lanes than a wave pair offers");
    if (own_steps && tab.S == 1 && desc.A.n_comp > 1) return no("per-block steps of one circuit with compiled Verilog-A devices");
  } else if (stru.block_threads != 64) return no("a block needs more than one wavefront of device slots");
  if (tab.max_mc > 8) return no("more than 8 MOSFET classes in a block");
  if (tab.Ssrc != 1) return no("per-sample source parameters");
  const bool wg_consts = own_steps && tab.S == 1 && desc.A.n_comp > 1;   // per-block steps: every workgroup gets the sources of ITS blocks only (checked there)
  if (!wg_consts && (stru.needed_src.size() > (size_t)P_MAXSRC || desc.A.known.size() + (size_t)stru.n_dev_src() > P_MAX_ENTRIES)) return no("more than 64 sources / known-node and source values per attempt");
  if (!(tab.S == 1 || desc.A.n_comp == 1)) return no("several blocks per sample in a multi-sample batch");
  if (desc.A.nb > 0 && (tab.S != 1 || desc.A.border_dev.size() > 8)) return no("bordered form: one sample and at most 8 devices on the border alone");
  for (const ClassMeta& m : stru.h_cms) if ((!desc.A.wide && m.nslots > 64) || m.nc > stru.lu_variant || m.n_work <= 0 || m.spare1 <= 0) return no("a block class does not fit the one-wave register path");
  if (ps.n_cu == 0) { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return no("hipGetDeviceProperties failed"); ps.n_cu = prop.multiProcessorCount; }
  const long nblk = (long)desc.A.n_comp * tab.S;
  const int bpw = persist_bpw(nblk);
  if (nblk > (long)bpw * ps.n_cu && !own_steps) return no("more blocks than resident wavefronts (4 per CU)");
  // p_grid_reduce: 8 group leaders sweep at most 32 member workgroups each
  if (!own_steps && (nblk + bpw - 1) / bpw > 256) return no("more than 256 workgroups in a grid-wide reduction");
  size_t npwl = 0; for (int i : stru.needed_src) npwl += desc.src[i].ts.size();
  if (!wg_consts && npwl > P_MAX_PWL) return no("piecewise-linear tables above 2048 points");
  return true;
}
// Blocks per workgroup of the device-resident stepper: four (one per wavefront), or two — one wave pair per CU, the other two
// wavefronts idle — for few, heavy blocks (compiled Verilog-A devices: 57 k instructions per evaluation and a 5 kB constant block
// per instance): they then spread over twice the CUs and do not share a CU's vector L1 four ways.
inline int ch_circuit::persist_bpw(long nblk) const {
  if (ps.n_cu > 0 && desc.A.wide && stru.wide_split && nblk <= 2L * ps.n_cu) return 2;
  return PW;
}
// Every sample of a batch (n_comp == 1) or every block of one circuit of independent blocks (S == 1) takes its own steps when
// the output is wanted on a common `saveat` grid: independent blocks ARE independent problems, a shared step size only makes
// each pay for the others' break points and dilutes its local error in the array-wide norm.  (Not for the bordered form.)
inline bool ch_circuit::persist_own_steps(const ch_tran_opts& o) const {
  return ((desc.A.n_comp == 1 && tab.S > 1) || (tab.S == 1 && desc.A.n_comp > 1 && desc.A.nb == 0 && !desc.A.wide)) && o.n_saveat > 0 && o.step_control != CH_STEPS_SHARED && !env_on(Env::LOCKSTEP);
}
inline size_t ch_circuit::persist_wave_doubles(bool wg_consts) const {
  const size_t n_ent = wg_consts ? (size_t)P_MAXSRC : desc.A.known.size() + stru.n_dev_src();
  return stru.lds_doubles_fixed + stru.lds_pad_doubles + 16 * (size_t)desc.A.max_nc + 10 + 48 + P_MAXSRC + n_ent + (size_t)tab.max_mc * (B4L_STRIDE + B4D_STRIDE) + (stru.lds_extra_bytes + stru.lds_plan_bytes + 7) / 8 + 2;
}
// Constants blob of the device stepper: needed sources, known-node definitions, device-source map, PWL tables.
// entries `kn` (known-node indices) then `ds` (device-source slots) -> blob; false when a limit of the kernel is exceeded
inline bool ch_circuit::persist_blob(const std::vector<int>& kn, const std::vector<int>& ds, std::vector<int>& bi, std::vector<double>& bd, std::vector<int>& need) const {
  const int nsrc = (int)desc.src.size();
  std::vector<char> nd(std::max(1, nsrc), 0);
  for (int k : kn) for (auto& tm : desc.A.known[k].terms) nd[tm.first] = 1;
  for (int j : ds) if (j < (int)stru.dev_src.size()) nd[stru.dev_src[j]] = 1;
  need.clear();
  for (int i = 0; i < nsrc; ++i) if (nd[i]) need.push_back(i);
  std::vector<int> pos(std::max(1, nsrc), -1);
  for (size_t i = 0; i < need.size(); ++i) pos[need[i]] = (int)i;
  std::vector<double> pt, py;
  bi = {(int)need.size(), (int)(kn.size() + ds.size()), 0, (int)kn.size()};
  for (int i : need) { bi.push_back(desc.src[i].kind); bi.push_back((int)pt.size()); bi.push_back((int)desc.src[i].ts.size()); pt.insert(pt.end(), desc.src[i].ts.begin(), desc.src[i].ts.end()); py.insert(py.end(), desc.src[i].ys.begin(), desc.src[i].ys.end()); }
  bi[2] = (int)pt.size();
  // entries: the known-node values, then the device source values (kvl and svl are contiguous in LDS)
  std::vector<int> eptr(1, 0), eidx; std::vector<double> ecoef;
  for (int k : kn) { for (auto& tm : desc.A.known[k].terms) { eidx.push_back(pos[tm.first]); ecoef.push_back(tm.second); } eptr.push_back((int)eidx.size()); }
  for (int j : ds) { if (j < (int)stru.dev_src.size()) { eidx.push_back(pos[stru.dev_src[j]]); ecoef.push_back(1.0); } eptr.push_back((int)eidx.size()); }
  bi.insert(bi.end(), eptr.begin(), eptr.end()); bi.insert(bi.end(), eidx.begin(), eidx.end());
  bd.clear();
  for (int i : need) for (int k = 0; k < CH_SRC_NPAR; ++k) bd.push_back(tab.src_par[(size_t)i * CH_SRC_NPAR + k]);
  bd.insert(bd.end(), ecoef.begin(), ecoef.end()); bd.insert(bd.end(), pt.begin(), pt.end()); bd.insert(bd.end(), py.begin(), py.end());
  for (size_t q = 4; q < bi.size(); ++q) if (bi[q] < 0) return false;
  return need.size() <= (size_t)P_MAXSRC && kn.size() + ds.size() <= P_MAX_ENTRIES && pt.size() <= P_MAX_PWL;
}

// The instantiations of tran_persistent_kernel, by (compiled Verilog-A stamps, mode, register-LU size, wave pairs); null: not built.
inline const void* persist_kernel(bool wide, int mode, int nc, bool pair) {
  struct Row { bool wide; int mode, nc; bool pair; const void* fn; };
  static const Row rows[] = {
    {true, PM_OWN, 16, true, (const void*)tran_persistent_kernel<16, true, PM_OWN, true>}, {true, PM_OWN, 16, false, (const void*)tran_persistent_kernel<16, false, PM_OWN, true>},
    {true, PM_LOCKSTEP, 16, true, (const void*)tran_persistent_kernel<16, true, PM_LOCKSTEP, true>}, {true, PM_LOCKSTEP, 16, false, (const void*)tran_persistent_kernel<16, false, PM_LOCKSTEP, true>},
    {false, PM_BORDER, 16, true, (const void*)tran_persistent_kernel<16, true, PM_BORDER>}, {false, PM_BORDER, 16, false, (const void*)tran_persistent_kernel<16, false, PM_BORDER>},
    {false, PM_OWN, 12, true, (const void*)tran_persistent_kernel<12, true, PM_OWN>}, {false, PM_OWN, 12, false, (const void*)tran_persistent_kernel<12, false, PM_OWN>},
    {false, PM_OWN, 16, true, (const void*)tran_persistent_kernel<16, true, PM_OWN>}, {false, PM_OWN, 16, false, (const void*)tran_persistent_kernel<16, false, PM_OWN>},
    {false, PM_LOCKSTEP, 12, true, (const void*)tran_persistent_kernel<12, true>}, {false, PM_LOCKSTEP, 12, false, (const void*)tran_persistent_kernel<12, false>},
    {false, PM_LOCKSTEP, 16, true, (const void*)tran_persistent_kernel<16, true>}, {false, PM_LOCKSTEP, 16, false, (const void*)tran_persistent_kernel<16, false>},
  };
  for (const Row& r : rows) if (r.wide == wide && r.mode == mode && r.nc == nc && r.pair == pair) return r.fn;
  return nullptr;
}

struct PersistConsts {
  std::vector<int> ci; std::vector<double> cd; size_t max_ci = 0, max_cd = 0;   // blob(s); layout sizes (the largest workgroup blob)
  std::vector<int> wgc, wgk;    // wg_consts: per workgroup {ci offset, cd offset, n_ci, n_cd, bps offset, nbp}; its entries' circuit-wide ids
  std::vector<double> bps_all;  // wg_consts: every workgroup's [times | codes]
};
// One blob for the whole grid, or — per-block steps of one circuit (wg_consts) — one per workgroup holding only what its
// blocks reference, with a map from the circuit's known-node / device-source indices to the workgroup's entries: a block with
// its own clock source neither evaluates nor stops at the other 1023 clocks.
inline bool ch_circuit::persist_consts(bool wg_consts, int n_wg, int bpw, const TranPlan& p, PersistConsts& pc) {
  const int nblk = desc.A.n_comp * tab.S, nk = (int)desc.A.known.size(), nds = stru.n_dev_src();
  if (!wg_consts) {
    std::vector<int> kn(nk), ds(nds), need;
    std::iota(kn.begin(), kn.end(), 0); std::iota(ds.begin(), ds.end(), 0);
    if (!persist_blob(kn, ds, pc.ci, pc.cd, need)) { set_err("device-resident stepper: the source tables exceed the kernel's limits"); return false; }
    pc.max_ci = pc.ci.size(); pc.max_cd = pc.cd.size();
  } else {
    pc.wgk.assign((size_t)n_wg * P_MAXSRC, -1);   // [wg][entry]: known-node index (entries 0 .. nk_local-1), then device-source slot
    for (int w = 0; w < n_wg; ++w) {
      std::vector<char> uk(nk, 0), ud(nds, 0);
      for (int b = w * bpw; b < std::min(nblk, (w + 1) * bpw); ++b)
        for (int i = 0; i < desc.A.comp_ndev[b]; ++i) {
          const EDev& e = desc.A.edev[desc.A.comp_dofs[b] + i];
          for (int k = 0; k < NTERM; ++k) if (e.term[k] < 0) uk[-e.term[k] - 1] = 1;
          if (e.src >= 0) ud[torn.dsrc_host[desc.A.comp_dofs[b] + i]] = 1;
        }
      std::vector<int> kn, ds, need, bi; std::vector<double> bd;
      for (int k = 0; k < nk; ++k) if (uk[k]) kn.push_back(k);
      for (int j = 0; j < nds; ++j) if (ud[j]) ds.push_back(j);
      if (ds.empty()) ds.push_back(0);   // the kernel's source-value array is never empty
      if (!persist_blob(kn, ds, bi, bd, need)) { set_err("device-resident stepper: a workgroup's blocks reference more than 64 sources / known nodes"); return false; }
      for (size_t q = 0; q < kn.size(); ++q) pc.wgk[(size_t)w * P_MAXSRC + q] = kn[q];
      for (size_t q = 0; q < ds.size(); ++q) pc.wgk[(size_t)w * P_MAXSRC + kn.size() + q] = ds[q];
      std::vector<double> wb, wc;
      collect_breakpoints(desc.src, tab.src_par, 1, p.t0, p.t1, wb, wc, &need);
      pc.wgc.insert(pc.wgc.end(), {(int)pc.ci.size(), (int)pc.cd.size(), (int)bi.size(), (int)bd.size(), (int)pc.bps_all.size(), (int)wb.size()});
      pc.ci.insert(pc.ci.end(), bi.begin(), bi.end()); pc.cd.insert(pc.cd.end(), bd.begin(), bd.end());
      pc.bps_all.insert(pc.bps_all.end(), wb.begin(), wb.end());
      pc.bps_all.insert(pc.bps_all.end(), wc.begin(), wc.end());   // the codes of these times follow them (the kernel reads code i at [count + i])
      pc.max_ci = std::max(pc.max_ci, bi.size()); pc.max_cd = std::max(pc.max_cd, bd.size());
    }
  }
  return true;
}

// Compiled Verilog-A devices: room for the workgroup's parameter and constant blocks in LDS (what the blocks of the heaviest
// component need, without counting shared blocks once; the kernel shares them and stops staging when the arena is full).
// Returns the arena in doubles and adds it to `lds` (bytes).
inline size_t ch_circuit::persist_va_arena(int bpw, size_t& lds) const {
  size_t va_arena = 0;
  if (desc.A.wide && !env_on(Env::VA_NO_LDS)) {
    size_t worst = 0;
    for (int cpt = 0; cpt < desc.A.n_comp; ++cpt) {
      size_t need = 0;
      for (int i = 0; i < desc.A.comp_ndev[cpt]; ++i) {
        const EDev& e = desc.A.edev[desc.A.comp_dofs[cpt] + i];
        if (e.kind != K_VA) continue;
        const int mod = desc.dev[e.hdev].ipar[0];
        need += (size_t)((va_gen::param_doubles(mod) + 1) & ~1) + (size_t)((va_gen::cache_doubles(mod) + 1) & ~1);
      }
      worst = std::max(worst, need);
    }
    const size_t room = lds < 148 * 1024 ? (148 * 1024 - lds) / sizeof(double) : 0;
    va_arena = std::min(worst * (size_t)bpw, room);
    lds += va_arena * sizeof(double);
    if (env_on(Env::DEBUG_STEPPER)) std::fprintf(stderr, "[stepper] compiled devices: %zu doubles per block, LDS arena %zu doubles, workgroup LDS %zu bytes\n", worst, va_arena, lds);
  }
  return va_arena;
}

// ---- what a launch reads and writes besides the state: constants up, one block of outputs and records, a pinned buffer ----
// Offsets (doubles) into DeviceStepper::d_pio: [times | point counts | workgroup records | group records | counters].  The kernel
// finds the point counts at out_times + max_rows; the records (16 granules each, double-buffered by generation parity) and the
// counters (10, on 128-byte lines) start on 256-byte boundaries.  Everything from `pts` to `end` is cleared before every launch.
struct PersistIo { size_t pts, wgrec, grprec, cnt, end; };
inline PersistIo persist_io_layout(long long max_rows, int n_wg) {
  PersistIo io;
  io.pts = (size_t)max_rows;
  io.wgrec = ((size_t)2 * max_rows + 31) & ~size_t(31);
  io.grprec = io.wgrec + (size_t)2 * n_wg * 16;
  io.cnt = io.grprec + 2 * 8 * 16;
  io.end = io.cnt + (10 * 32 * sizeof(unsigned) + sizeof(double) - 1) / sizeof(double);
  return io;
}
// How a step of the device stepper's driver ended.  Declined: nothing was launched and err() says why this circuit, this request
// or the GPU at this moment does not take it.  Failed: an error (rc) in front of the first launch.  Ready: persist_prepare has
// filled the launch record; from persist_run, the kernel was launched, and rc is CH_OK or an error behind that launch.
// try_device_stepper treats Declined and Failed alike — the host stepper takes the transient, with err() as the reason —
// while dc_border returns a Failed step's rc as it is (and CH_ERR_UNSUPPORTED for Declined).
enum class PersistOutcome { Declined, Failed, Ready };
struct PersistStep {
  PersistOutcome what; int rc;
  PersistStep(int rc_) : what(rc_ == CH_OK ? PersistOutcome::Ready : PersistOutcome::Failed), rc(rc_) {}   // (what HIPCHK returns)
  PersistStep(PersistOutcome w, int rc_) : what(w), rc(rc_) {}
  static PersistStep declined() { return {PersistOutcome::Declined, CH_OK}; }
  bool launched() const { return what == PersistOutcome::Ready; }
};
// Everything persist_prepare decides for one call: the grid, the LDS, the row buffer, the kernel and its arguments.
struct PersistLaunch {
  int nblk = 0, bpw = 0, n_wg = 0; bool own_steps = false, wg_consts = false, pair = false, coop = false;
  size_t wave_d = 0, lds = 0, va_arena = 0, row_d = 1; long long max_rows = 0;
  PersistIo io{}; const void* fn = nullptr; PersistArgs pa;
};
// What persist_run brings back: the controller's exit state, the solve's status, the rows (single_batch: the values are in the
// result already, transposed on the device, and xs_final is the final state; otherwise hrows holds the drained batches), and the
// device time of its launches.
struct PersistRun {
  TranCtl cs; int status = CH_OK; bool single_batch = false;
  std::vector<double> hrows, htimes, hpts, xs_final;
  double device_ms = 0; long launches = 0;
};
// The pinned buffer: the controller state in and out in front (P_CTL_D doubles each), behind them the constants on their way
// up or the read-back of a finished launch.  Growing drops the contents: only with nothing in flight.
constexpr size_t P_CTL_D = (sizeof(TranCtl) + sizeof(double) - 1) / sizeof(double);
constexpr size_t P_PINNED_VALUES = size_t(1) << 20;   // results up to this many doubles come back through the pinned buffer
inline int ch_circuit::persist_stage(size_t doubles) {
  if (ps.h_stage.n >= doubles) return CH_OK;
  HIPCHK(ps.h_stage.alloc(std::max(doubles, 2 * ps.h_stage.n)));
  return CH_OK;
}
// One constant array of the launch: (re)allocated when it grew, and listed for upload when its buffer is new or holds something else.
struct ConstCopy { void* dst; const void* src; size_t bytes; };
template <class T>
inline hipError_t persist_const(DevBuf<T>& d, std::vector<T>& held, const std::vector<T>& now, std::vector<ConstCopy>& copies) {
  bool fresh = false;
  if (now.size() > d.n || !d.p) { const hipError_t e = d.alloc(now.size()); if (e != hipSuccess) return e; fresh = true; }
  const size_t bytes = now.size() * sizeof(T);
  if (!fresh && held.size() == now.size() && (bytes == 0 || std::memcmp(held.data(), now.data(), bytes) == 0)) return hipSuccess;
  held = now;
  if (bytes) copies.push_back({d.p, held.data(), bytes});
  return hipSuccess;
}
// The constants of a launch — blob(s), break points with their codes, the output grid, the per-workgroup maps — are the same from
// transient to transient on one circuit and one time span: each array is compared (bit for bit) with what its buffer received
// last and skipped when equal.  What did change goes through the pinned buffer in asynchronous copies; the launch is ordered behind them.
inline int ch_circuit::persist_upload_consts(const PersistConsts& pc, const std::vector<double>& bpu, const std::vector<double>& sv, bool wg_consts) {
  std::vector<ConstCopy> copies;
  hipError_t e = persist_const(ps.d_pci, ps.h_pci, pc.ci, copies);
  if (e == hipSuccess) e = persist_const(ps.d_pcd, ps.h_pcd, pc.cd, copies);
  if (e == hipSuccess) e = persist_const(ps.d_pbps, ps.h_pbps, bpu, copies);
  if (e == hipSuccess && wg_consts) e = persist_const(ps.d_pwgc, ps.h_pwgc, pc.wgc, copies);
  if (e == hipSuccess && wg_consts) e = persist_const(ps.d_pwgk, ps.h_pwgk, pc.wgk, copies);
  if (e == hipSuccess) e = persist_const(ps.d_psave, ps.h_psave, sv, copies);
  size_t total = 0, at = 2 * P_CTL_D;
  for (const ConstCopy& c : copies) total += (c.bytes + sizeof(double) - 1) / sizeof(double);
  if (e == hipSuccess && total > 0 && ps.h_stage.n < at + total) e = ps.h_stage.alloc(std::max(at + total, 2 * ps.h_stage.n));
  for (size_t i = 0; i < copies.size() && e == hipSuccess; ++i) {
    std::memcpy(ps.h_stage.p + at, copies[i].src, copies[i].bytes);
    e = hipMemcpyAsync(copies[i].dst, ps.h_stage.p + at, copies[i].bytes, hipMemcpyHostToDevice, ctx->stream);
    at += (copies[i].bytes + sizeof(double) - 1) / sizeof(double);
  }
  if (e != hipSuccess) {
    // what the buffers hold is unknown now: the next call uploads everything
    ps.h_pci.clear(); ps.h_pcd.clear(); ps.h_pbps.clear(); ps.h_pwgc.clear(); ps.h_pwgk.clear(); ps.h_psave.clear();
    set_err(std::string("device-resident stepper: constants: ") + hipGetErrorString(e)); return CH_ERR_DEVICE;
  }
  return CH_OK;
}
// The whole transient in one launch: the times, the point counts, the rows — transposed on the device into the result's layout
// [observable][time][sample], so that they cross PCIe once (the host-side transposition of a result with every node observed,
// 100 MB for the 1024-DFF array, cost several times the solve) — and the final state (ring slot 0) are enqueued together and
// waited for once.  Asynchronous copies need pinned memory: results of up to P_PINNED_VALUES doubles take the pinned buffer,
// larger ones land in the result directly as before.
inline int ch_circuit::persist_readback(ch_result& R, size_t nt, const PersistIo& io, PersistRun& out) {
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)R.n_obs * nt * tab.S, nx = (size_t)tab.S * desc.A.n_unk;
  const bool pinned_values = n <= P_PINNED_VALUES;
  R.values.assign(n, 0.0);
  { const int rcs = persist_stage(2 * P_CTL_D + 2 * nt + nx + (pinned_values ? n : 0)); if (rcs != CH_OK) return rcs; }
  double* const h_t = ps.h_stage.p + 2 * P_CTL_D; double* const h_p = h_t + nt; double* const h_x = h_p + nt; double* const h_v = h_x + nx;
  if (nt > 0) {
    HIPCHK(hipMemcpyAsync(h_t, ps.d_pio.p, nt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_p, ps.d_pio.p + io.pts, nt * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (n > 0) {
    HIPCHK(ps.d_ptrans.alloc(n));
    hipLaunchKernelGGL(transpose_rows_kernel, dim3((unsigned)std::min<size_t>(65535, (n + 255) / 256)), dim3(256), 0, st, (const double*)ps.d_prows.p, ps.d_ptrans.p, (long)nt, (long)R.n_obs, tab.S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(pinned_values ? h_v : R.values.data(), ps.d_ptrans.p, n * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (nx > 0) HIPCHK(hipMemcpyAsync(h_x, nwt.d_X.p, nx * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  out.htimes.assign(h_t, h_t + nt); out.hpts.assign(h_p, h_p + nt); out.xs_final.assign(h_x, h_x + nx);
  if (pinned_values) std::copy(h_v, h_v + n, R.values.begin());
  return CH_OK;
}

// Statistics and rows of a finished transient on the device stepper -> the result (then finish_tran).  single_batch: persist_readback
// has filled the result's values (the transposed rows stay on the device) and read the final state; otherwise `hrows` holds the
// drained batches.
inline int ch_circuit::persist_collect(ch_result& R, const PersistRun& out, bool own_steps, hclock::time_point tstart) {
  LapTimer lt(host_profile);
  const TranCtl& cs = out.cs;
  const int n_obs = R.n_obs;
  stats.persist_attempts = cs.n_attempts;
  stats.persist_barrier_s = (double)cs.t_cycles_barrier * 1e-8;
#ifdef CH_STAMPS
  { static const char* nm[12] = {"set-up", "coefficients", "sources", "predictor", "eval", "gather", "rows+norm", "LU+solves", "update", "candidate", "grid-reduce", "controller"};
    std::fprintf(stderr, "[pstamps] attempts %lld; cycles per attempt (wave 0 of workgroup 0):", cs.n_attempts);
    for (int q = 0; q < 12; ++q) std::fprintf(stderr, " %s %.0f", nm[q], (double)cs.stamps[q] / (double)std::max<long long>(1, cs.n_attempts));
    std::fprintf(stderr, "\n"); }
#endif
  R.stats.naccept += cs.naccept; R.stats.nreject += cs.nreject; R.stats.nnonlinconvfail += cs.nconvfail;
  const long long arr_iters = (own_steps && tab.S == 1) ? cs.max_iters : cs.sum_iters;   // one circuit: Newton iterations of its slowest block
  add_newton_iters(R.stats, arr_iters, cs.sum_block_iters);
  const size_t nt = out.htimes.size();
  R.times = out.htimes;
  R.pts.assign(nt, 0);
  if (!own_steps) for (size_t r = 0; r < nt; ++r) R.pts[r] = (int32_t)out.hpts[r];
  if (out.single_batch) {
    const size_t n = (size_t)n_obs * nt * tab.S;
    if (n > 0) {
      // the rows stay in HBM for a device-side consumer (the RCCL gather of a sharded sweep) when every observable is a plain
      // unknown — the host-side fix-ups of finish_tran (merged nodes, known nodes, eliminated branches) do not reach this buffer
      bool plain = true;
      for (int ob = 0; ob < n_obs && plain; ++ob) {
        if (stru.obs_primary[ob] != ob) plain = false;
        else if (desc.obs_kind[ob] == 0 && desc.A.node_unknown[desc.obs_index[ob]] < 0) plain = false;
        else if (desc.obs_kind[ob] == 1) { const int br = desc.dev[desc.obs_index[ob]].branch; if (br < 0 || desc.A.branch_unknown[br] < 0) plain = false; }
      }
      if (plain) { R.dev_values = ps.d_ptrans.p; R.dev_n = (int64_t)n; }
    }
  } else {
    R.values.assign((size_t)n_obs * nt * tab.S, 0.0);
    rows_to_obs_major(out.hrows.data(), nt, 0, nt, n_obs, tab.S, R.values.data());
  }
  lt.lap(laps.collect);
  return finish_tran(R, 0, cs.t, out.status, tstart, out.single_batch ? out.xs_final.data() : nullptr);
}

// ---- prepare: everything in front of the first launch ----
// The kernel's arguments.  dcm: the operating point of the bordered form instead of a transient (PersistArgs::dc_mode) — the state
// in ring slot 0 is the initial iterate and receives the result.
inline int ch_circuit::persist_fill_args(const TranPlan& p, const ch_dc_opts* dcm, PersistLaunch& L) {
  const ch_tran_opts& o = *p.o;
  const int nk = (int)desc.A.known.size(), nds = stru.n_dev_src();
  PersistArgs& pa = L.pa; std::memset(&pa, 0, sizeof(pa));
  pa.a = nwt.base;
  pa.a.mode = MODE_TRAN; pa.a.maxit = p.nmaxit; pa.a.abstol = o.abstol; pa.a.reltol = o.reltol; pa.a.newton_tol = 0.1; pa.a.active = nullptr; pa.a.gshunt = 0.0;
  pa.bpw = L.bpw; pa.wide_l = stru.wide_l; pa.wide_other = stru.wide_other; pa.va_arena = (int)L.va_arena;
  pa.nblk = L.nblk; pa.n_wg = L.n_wg; pa.red_max = (tab.S > 1 || L.own_steps) ? 1 : 0; pa.wave_doubles = (int)L.wave_d;
  pa.t1 = p.t1; pa.dtmin = p.dtmin; pa.dtmax = p.dtmax; pa.first_frac = FIRST_STEP_FRAC; pa.kmax = p.kmax; pa.max_steps = p.max_steps;
  pa.bps = ps.d_pbps.p; pa.nbp = (int)p.bps.size(); pa.saveat = ps.d_psave.p; pa.n_saveat = o.n_saveat;
  pa.ci = ps.d_pci.p; pa.cd = ps.d_pcd.p;
  pa.wgc = L.wg_consts ? ps.d_pwgc.p : nullptr; pa.wgk = L.wg_consts ? ps.d_pwgk.p : nullptr;
  pa.out_times = ps.d_pio.p; pa.out_rows = ps.d_prows.p; pa.max_rows = L.max_rows; pa.n_obs = (int)desc.obs_kind.size();
  pa.ctl = ps.d_pctl.p; pa.wg_rec = ps.d_pio.p + L.io.wgrec; pa.grp_rec = ps.d_pio.p + L.io.grprec; pa.counters = (unsigned*)(ps.d_pio.p + L.io.cnt);
  pa.spin_ticks = 200000000LL;   // 2 s at 100 MHz
  if (env_on(Env::SPIN_TICKS)) pa.spin_ticks = std::max(1L, env_long(Env::SPIN_TICKS, 0));   // test hook: makes every wait give up (exercises the fallback)
  // a batch of single-block samples on a common output grid: every sample its own step sequence (no lock-step, no grid reduction)
  pa.indep = L.own_steps ? 1 : 0;
  ps.mode = desc.A.nb > 0 ? CH_MODE_BORDERED : (L.own_steps ? CH_MODE_OWN_STEPS : CH_MODE_LOCKSTEP);
  if (dcm) {
    if (desc.A.nb == 0 || L.wg_consts) { set_err("internal: operating point on the device stepper is for the bordered form"); return CH_ERR_INTERNAL; }
    std::vector<double> sv, kv, ent;
    eval_sources(0.0, dcm->tran_mode ? 2 : 0, sv, kv);
    ent.assign(kv.begin(), kv.begin() + nk); ent.insert(ent.end(), sv.begin(), sv.begin() + nds);
    HIPCHK(ps.d_pdcent.upload(ent, ctx->stream));
    pa.dc_mode = 1; pa.dc_maxit = std::max(1, dcm->maxiters); pa.dc_abstol = dcm->abstol; pa.dc_entries = ps.d_pdcent.p;
    pa.dv_max = (!desc.A.mos_hdev.empty() || desc.A.wide) ? dcm->dv_max : 0.0;   // linear circuits take the full Newton step (as on the other paths)
  }
  pa.nb = desc.A.nb; pa.n_glob = desc.A.n_glob; pa.n_bdev = (int)desc.A.border_dev.size();
  for (int q = 0; q < pa.n_bdev; ++q) {
    const Analysis::BorderDev& bd = desc.A.border_dev[q];
    pa.bd_kind[q] = bd.kind; pa.bd_ta[q] = bd.ta; pa.bd_tb[q] = bd.tb;
    const double par0 = tab.dpar[(size_t)bd.hdev * tab.Spar], mult0 = tab.dmult[(size_t)bd.hdev * tab.Spar];   // sample 0 of the tables as uploaded
    pa.bd_val[q] = bd.kind == K_R ? mult0 / par0 : mult0 * par0;
  }
  pa.pair_dbg = (int)env_long(Env::PAIR_DBG, 0);
  return CH_OK;
}
// the instantiation for this form; its static LDS and its dynamic-LDS ceiling: read and raised once per function (the ceiling does not depend on the call)
inline PersistStep ch_circuit::persist_pick_kernel(PersistLaunch& L) {
  const int mode = desc.A.wide ? (L.own_steps ? PM_OWN : PM_LOCKSTEP) : desc.A.nb > 0 ? PM_BORDER : (L.own_steps ? PM_OWN : PM_LOCKSTEP);
  L.fn = persist_kernel(desc.A.wide, mode, persist_lu_nc(desc.A.wide, desc.A.nb, desc.A.max_nc), L.pair);   // (the size the gather schedule's strides were built for)
  if (!L.fn) { set_err("internal: no device-stepper kernel for this form"); return CH_ERR_INTERNAL; }
  if (ps.attr_fn != L.fn) {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, L.fn));
    if (fa.sharedSizeBytes <= LDS_BYTES_PER_CU) HIPCHK(hipFuncSetAttribute(L.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_dynamic_ceiling((int)fa.sharedSizeBytes)));
    ps.attr_static_lds = fa.sharedSizeBytes; ps.attr_fn = L.fn;
  }
  if (L.lds + ps.attr_static_lds > LDS_BYTES_PER_CU) { set_err("device-resident stepper: LDS footprint"); return PersistStep::declined(); }
  return CH_OK;
}
// Eligibility of the blob and the LDS sizing, the constants' upload and the allocations, then the arguments and the kernel.
inline PersistStep ch_circuit::persist_prepare(const TranPlan& p, const ch_dc_opts* dcm, PersistLaunch& L) {
  const ch_tran_opts& o = *p.o;
  g_arena = &arena;
  LapTimer lt(host_profile);
  L.nblk = desc.A.n_comp * tab.S; L.bpw = persist_bpw(L.nblk); L.n_wg = (L.nblk + L.bpw - 1) / L.bpw;
  L.own_steps = persist_own_steps(o);
  L.wg_consts = L.own_steps && tab.S == 1 && desc.A.n_comp > 1;
  PersistConsts pc;
  if (!persist_consts(L.wg_consts, L.n_wg, L.bpw, p, pc)) return PersistStep::declined();
  L.wave_d = persist_wave_doubles(L.wg_consts);
  L.lds = (pc.max_cd + (pc.max_ci + 1) / 2 + PW * P_NREC + P_NREC + 4 + P_SCR + PW * L.wave_d) * sizeof(double);
  L.va_arena = persist_va_arena(L.bpw, L.lds);
  // wave pairs share the device evaluation by function when every block has the same class and at most 32 evaluation slots
  L.pair = desc.A.wide ? stru.wide_split : (desc.A.classes.size() == 1 && stru.h_cms[0].nslots <= 32 && !env_on(Env::PERSIST_NOPAIR));
  if (L.lds > 150 * 1024) { set_err("device-resident stepper: the workgroup's LDS footprint exceeds 150 KB"); return PersistStep::declined(); }
  // ---- output rows (the operating point saves none) ----
  L.row_d = std::max<size_t>(1, desc.obs_kind.size() * (size_t)tab.S);
  const bool force = o.n_saveat == 0 && env_on(Env::PERSIST_MAXROWS);
  const long forced = force ? env_long(Env::PERSIST_MAXROWS, 0) : 0;
  L.max_rows = dcm ? 2 : persist_max_rows(o.n_saveat, p.max_steps, L.row_d, force ? &forced : nullptr);
  {
    std::vector<double> bpu = L.wg_consts ? pc.bps_all : p.bps;   // [times | codes]
    if (!L.wg_consts) bpu.insert(bpu.end(), p.bpc.begin(), p.bpc.end());
    std::vector<double> sv(o.saveat, o.saveat + std::max(0, o.n_saveat)); if (sv.empty()) sv.push_back(0.0);
    const int rcu = persist_upload_consts(pc, bpu, sv, L.wg_consts);
    if (rcu != CH_OK) return rcu;
  }
  L.io = persist_io_layout(L.max_rows, L.n_wg);
  HIPCHK(ps.d_pio.alloc(L.io.end)); HIPCHK(ps.d_prows.alloc((size_t)L.max_rows * L.row_d));
  HIPCHK(ps.d_pctl.alloc(2));   /* controller state in; [1]: exit state of a batch with per-sample steps */
  { const int rca = persist_fill_args(p, dcm, L); if (rca != CH_OK) return rca; }
  L.pa.n_ci = (int)pc.max_ci; L.pa.n_cd = (int)pc.max_cd;   // layout sizes (the largest workgroup blob)
  // Own steps: no grid-wide wait anywhere in the kernel, so the workgroups need not be co-resident — an ordinary launch whose
  // workgroups may queue (behind each other, or behind another process's kernel: a cooperative launch would be refused there)
  L.coop = !L.pa.indep;
  { const PersistStep k = persist_pick_kernel(L); if (k.what != PersistOutcome::Ready) return k; }
  { const int rcs = persist_stage(2 * P_CTL_D); if (rcs != CH_OK) return rcs; }
  lt.lap(laps.consts);
  return CH_OK;
}

// ---- run: launch, wait, read back, resume while the row buffer fills ----
// One launch behind the controller state `cs`; `refused`: what the launch call itself answered
inline int ch_circuit::persist_launch(PersistLaunch& L, const TranCtl& cs, int resume, hipError_t& refused) {
  hipStream_t st = ctx->stream;
  // controller state in and out through the pinned buffer: [0] in, [1] out (the constants' copies behind them are long consumed
  // when the read-back reuses that room: the wait of persist_drain lies between)
  TranCtl* const h_in = (TranCtl*)ps.h_stage.p;
  *h_in = cs;
  HIPCHK(hipMemcpyAsync(ps.d_pctl.p, h_in, sizeof(cs), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ps.d_pctl.p + 1, h_in, sizeof(cs), hipMemcpyHostToDevice, st));
  // ONE clear: point counts, workgroup and group records (generation tags start at 0), counters
  HIPCHK(hipMemsetAsync(ps.d_pio.p + L.io.pts, 0, (L.io.end - L.io.pts) * sizeof(double), st));
  // own steps: a block that stops early (DtLessThanMin, MaxIters) never writes its later saveat rows; they read as NaN
  if (L.pa.indep) HIPCHK(hipMemsetAsync(ps.d_prows.p, 0xff, (size_t)L.max_rows * L.row_d * sizeof(double), st));
  L.pa.resume = resume;
  void* kargs[] = {(void*)&L.pa};
  HIPCHK(hipEventRecord(nwt.ev0, st));
  refused = L.coop ? hipLaunchCooperativeKernel(L.fn, dim3(L.n_wg), dim3(PW * 64), kargs, (unsigned)L.lds, st)
                   : hipLaunchKernel(L.fn, dim3(L.n_wg), dim3(PW * 64), kargs, L.lds, st);
  if (refused != hipSuccess) { (void)hipGetLastError(); return CH_OK; }
  HIPCHK(hipEventRecord(nwt.ev1, st));
  return CH_OK;
}
// The waits behind a launch: its exit state -> out.cs, then its rows.  R: the result whose values a whole transient in one launch
// fills directly (null: the operating point, which has none)
inline int ch_circuit::persist_drain(const PersistLaunch& L, ch_result* R, int resume, PersistRun& out, LapTimer& lt) {
  hipStream_t st = ctx->stream;
  const TranCtl* const h_out = (const TranCtl*)(ps.h_stage.p + P_CTL_D);
  TranCtl& cs = out.cs;
  // first wait: the launch and, behind it, its exit state
  { hipError_t se = hipMemcpyAsync((void*)h_out, ps.d_pctl.p + (L.pa.indep ? 1 : 0), sizeof(cs), hipMemcpyDeviceToHost, st);
    if (se == hipSuccess) se = hipStreamSynchronize(st);
    if (se != hipSuccess) { set_err(std::string("device-resident stepper: ") + hipGetErrorString(se)); return CH_ERR_DEVICE; } }
  { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, nwt.ev0, nwt.ev1)); out.device_ms += ms; out.launches += 1; }
  cs = *h_out;
  lt.lap(laps.launch_sync);
  // rows of this launch
  const size_t nr = (size_t)cs.nsaved, base_t = out.htimes.size(), row_d = L.row_d;
  // The usual case — the whole transient in one launch: the rows are transposed on the device into the result's layout
  // [observable][time][sample] and cross PCIe once, straight into the result (the host-side transposition of a result with
  // every node observed, 100 MB for the 1024-DFF array, cost several times the solve).  Drained batches keep the host path.
  out.single_batch = resume == 0 && cs.exit_reason != PX_ROWS_FULL && R;
  out.htimes.resize(base_t + nr); out.hpts.resize(base_t + nr);
  if (!out.single_batch) out.hrows.resize((base_t + nr) * row_d);
  if (out.single_batch) {
    // second wait: times, point counts, the transposed rows and the final state in one batch
    const int rcb = persist_readback(*R, nr, L.io, out);
    if (rcb != CH_OK) return rcb;
  } else if (nr > 0) {
    HIPCHK(hipMemcpy(out.htimes.data() + base_t, ps.d_pio.p, nr * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.hpts.data() + base_t, ps.d_pio.p + L.io.pts, nr * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.hrows.data() + base_t * row_d, ps.d_prows.p, nr * row_d * sizeof(double), hipMemcpyDeviceToHost));
  }
  lt.lap(laps.readback);
  return CH_OK;
}
// A launch refused with nothing launched yet declines (the host stepper can take it); a refused relaunch, and any error behind
// the first launch, is a device error of a solve that ran.
inline PersistStep ch_circuit::persist_run(PersistLaunch& L, const TranPlan& p, ch_result* R, PersistRun& out) {
  // initial controller state (the host stepper's first step: start_step, ch_stepper_host.hpp)
  TranCtl& cs = out.cs; std::memset(&cs, 0, sizeof(cs));
  cs.t = p.t0; cs.h = start_step(p.o->dt0, p.t0, p.t1, p.dtmin, p.dtmax, p.bps[0]); cs.k = 1; cs.nhist = 1; cs.reset_rate = 1; cs.tslot[0] = p.t0;
  LapTimer lt(host_profile);
  bool launched = false;
  for (int resume = 0;; resume = 1) {
    hipError_t refused = hipSuccess;
    int rc = persist_launch(L, cs, resume, refused);
    if (rc == CH_OK && refused != hipSuccess) {
      if (resume == 0) { set_err(std::string("cooperative launch refused: ") + hipGetErrorString(refused)); return PersistStep::declined(); }
      set_err(std::string("device-resident stepper: relaunch failed: ") + hipGetErrorString(refused)); rc = CH_ERR_DEVICE;
    }
    if (rc == CH_OK) { launched = true; rc = persist_drain(L, R, resume, out, lt); }
    if (rc != CH_OK) return launched ? PersistStep(PersistOutcome::Ready, rc) : PersistStep(rc);
    if (cs.exit_reason != PX_ROWS_FULL) break;
    cs.nsaved = 0;   // the row buffer was full and has been drained: the next launch resumes
  }
  out.status = cs.status;
  if (cs.exit_reason == PX_ABORT) {
    ps.aborted = true;
    unsigned code = 0; (void)hipMemcpy(&code, (const unsigned*)(ps.d_pio.p + L.io.cnt) + 9 * 32, sizeof(code), hipMemcpyDeviceToHost);
    set_err("device-resident stepper: a wait exceeded its bound (site " + std::to_string(code & 255u) + ", sequence " + std::to_string(code >> 8) +
            ", attempts " + std::to_string((long long)cs.n_attempts) + "; workgroups not co-resident?)");
    out.status = CH_ERR_DEVICE;
  }
  return CH_OK;
}

// A transient on the device stepper: prepare -> run -> persist_collect.  Ready: rc is the transient's result
inline PersistStep ch_circuit::tran_persistent(const TranPlan& p, ch_result& R, hclock::time_point tstart) {
  PersistLaunch L; PersistRun out;
  PersistStep s = persist_prepare(p, nullptr, L);
  if (s.what != PersistOutcome::Ready) return s;
  s = persist_run(L, p, &R, out);
  stats.persist_ms += out.device_ms; stats.persist_launches += out.launches;
  if (s.launched() && s.rc == CH_OK) s.rc = persist_collect(R, out, L.own_steps, tstart);
  return s;
}

// Operating point of the torn form on the device stepper: ONE damped Newton solve (CedarDCOp's first attempt: from o.x0 or
// 1e-7*randn) with the Schur complement on the border per iteration.  Any other outcome than CH_OK sends the caller to the
// sparse path's full CedarDCOp (restarts, gmin stepping).  The result stays in ring slot 0 of THIS (torn) circuit.  The kernel
// runs it as one order-1 step over (0, 1) that saves no rows; its device time is the operating point's, not a transient's.
inline int ch_circuit::dc_border(const ch_dc_opts& o, long long* iters) {
  const auto td0 = hclock::now();
  auto lap = [&](const char* what) { if (env_on(Env::DEBUG_TORN)) std::fprintf(stderr, "[torn] dc_border %s at %.3f ms\n", what, 1e3 * std::chrono::duration<double>(hclock::now() - td0).count()); };
  int rc = finalize_params();
  if (rc != CH_OK) return rc;
  lap("finalized");
  std::string why;
  if (!torn.is_torn || !persist_eligible(why, false)) { set_err("bordered operating point: " + why); return CH_ERR_UNSUPPORTED; }
  std::vector<double> xm((size_t)tab.S * desc.A.n_mna, 0.0);
  if (o.x0) std::copy(o.x0, o.x0 + xm.size(), xm.begin());
  else { Rng rng(o.seed); for (double& v : xm) v = 1e-7 * rng.normal(); }
  lap("start vector");
  rc = upload_from_mna(0, xm.data());
  if (rc != CH_OK) return rc;
  lap("uploaded");
  ch_tran_opts to; ch_tran_opts_default(&to);   // the tolerances of the default request; no grid, no dt0
  TranPlan p;
  p.t0 = 0.0; p.t1 = 1.0; p.kmax = 1; p.dtmin = 1e-15; p.dtmax = 0.1; p.max_steps = 10; p.nmaxit = 10; p.bps = {1.0}; p.bpc = {-1.0}; p.o = &to;
  PersistLaunch L; PersistRun out;
  const auto tq0 = hclock::now();
  PersistStep s = persist_prepare(p, &o, L);
  if (s.what == PersistOutcome::Ready) s = persist_run(L, p, nullptr, out);
  if (env_on(Env::DEBUG_TORN)) std::fprintf(stderr, "[torn] dc_border: kernel %.3f ms, call %.3f ms\n", out.device_ms, 1e3 * std::chrono::duration<double>(hclock::now() - tq0).count());
  if (s.what == PersistOutcome::Declined) return CH_ERR_UNSUPPORTED;
  if (s.rc != CH_OK) return s.rc;
  if (iters) *iters = out.cs.sum_iters;
  return out.status;
}

// A coupled array behind a border of one or two unknowns: operating point and transient on the torn companion's device-resident
// stepper (operating point on this circuit's sparse path when the single damped Newton solve there does not converge).
// used = false: the companion does not take the problem (reason in torn.note).
inline int ch_circuit::tran_torn(double t0, double t1, const ch_tran_opts& o, ch_result& R, bool& used) {
  used = false;
  auto tstart = hclock::now();
  int rc = finalize_params();
  if (rc != CH_OK) return rc;
  std::vector<double> x_mna((size_t)tab.S * desc.A.n_mna, 0.0);
  ch_stats dcst; std::memset(&dcst, 0, sizeof(dcst));
  stats.reset();
  ch_circuit* tc = torn.c.get();
  bool dc_on_torn = false;
  if (o.skip_dc) { if (o.dc.x0) std::copy(o.dc.x0, o.dc.x0 + x_mna.size(), x_mna.begin()); }
  else {
    if (!env_on(Env::TORN_DC_SPARSE)) {
      long long it = 0;
      ArenaScope sc(&tc->arena);
      const int r = tc->dc_border(o.dc, &it);
      if (r == CH_OK) { dc_on_torn = true; add_newton_iters(dcst, it, it * tc->desc.A.n_comp); }
      else { torn.note = "bordered operating point: " + err(); ctx->err.clear(); }
      if (env_on(Env::DEBUG_TORN)) std::fprintf(stderr, "[torn] operating point on the device stepper: rc %d, %lld iterations, %.3f ms%s%s\n", r, it,
                                                           1e3 * std::chrono::duration<double>(hclock::now() - tstart).count(), r == CH_OK ? "" : " -> sparse path: ", r == CH_OK ? "" : torn.note.c_str());
    }
    if (!dc_on_torn) {
      rc = dc_solve(o.dc, 0, nullptr, &dcst);
      if (rc != CH_OK) { used = true; return rc; }
      rc = download_mna(0, t0, 1, x_mna.data());
      if (rc != CH_OK) return rc;
    }
  }
  const double dc_s = std::chrono::duration<double>(hclock::now() - tstart).count();
  const long dc_l = stats.n_launch;
  ch_tran_opts o2 = o; o2.skip_dc = 1; o2.dc.x0 = dc_on_torn ? nullptr : x_mna.data(); o2.stepper = CH_STEPPER_DEVICE;
  { ArenaScope sc(&tc->arena); tc->torn.keep_slot0 = dc_on_torn; rc = tc->tran_solve(t0, t1, o2, R); tc->torn.keep_slot0 = false; }
  if (rc == CH_ERR_UNSUPPORTED || (rc == CH_ERR_DEVICE && tc->ps.aborted)) { torn.note = err(); ctx->err.clear(); return CH_OK; }   // the sparse path takes it
  used = true;
  R.stats.dc_seconds = dc_s; R.stats.wall_seconds += dc_s; R.stats.n_kernel_launches += dc_l;
  add_newton_iters(R.stats, dcst.nnonliniter, dcst.n_block_iters); R.stats.nrestarts += dcst.nrestarts;   // (either operating point counted every iteration five ways)
  return rc;
}
