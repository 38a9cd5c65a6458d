// ch_engine_ac.hpp — small-signal analyses (AC, noise): what the whole family shares with the sensitivities of ch_engine_sens.hpp (the
// MODE_EVAL launch, the dense dumps at the operating point, the frequency check, the timing bracket of the launchers and the LDS
// budget of the LDS-resident solve kernels), the AC right-hand side, the dense complex solves (ac_block_kernel) and the two
// entry-point bodies, each a device half and a finish (ac_device_solve, ac_finish).  Included by ch_engine.hip behind the definition of ch_circuit.
#pragma once

// Small-signal analyses see the circuit as dense blocks: the Jacobian blocks of the fused path, or — on the sparse path —
// the whole system as one block per sample (up to 96 unknowns the complex LU runs in LDS, above that in a global workspace)
inline const BlockMeta* ch_circuit::ac_bmeta() {
  if (nwt.path != 2) return tab.d_bmeta.p;
  BlockMeta b; std::memset(&b, 0, sizeof(b)); b.uofs = 0; b.dofs = 0; b.cm.nc = desc.A.n_unk; b.cm.ndev = (int)desc.A.edev.size();
  std::vector<BlockMeta> v(1, b);
  g_arena = &arena;
  if (ac.d_bmeta_all.upload(v, ctx->stream) != hipSuccess) return nullptr;
  return ac.d_bmeta_all.p;
}

// ---- shared by AC, noise and both sensitivities ------------------------------------------------
// One MODE_EVAL launch at the state in ring slot `x_slot` (0: the operating point) with the tables of `a`, the source tables `src` and
// lds_extra bytes of dynamic LDS on top of the circuit's; F lands in dumpF as dense per-block vectors, G in dumpG and — when dumpC is
// given — C in dumpC (dumpC == nullptr: the launch is after the residual alone and dumpG is a scratch).  The transient sensitivities
// (ch_engine_transens.hpp) evaluate at a source time t, send the launch's candidate row to the ring slot cand_slot that is free between
// attempts (the small-signal analyses leave it at slot 1) and keep the charges: dumpQ, dense per block like dumpF
static int smallsignal_eval(ch_circuit* c, NewtonArgs a, SourceTables src, size_t lds_extra, int mode, double* dumpF, double* dumpG, double* dumpC, int x_slot = 0,
                            int cand_slot = 1, double t = 0.0, double* dumpQ = nullptr) {
  const int S = c->tab.S, ds = c->ac_ds();
  int rc = c->set_sources(a, t, mode, src);
  if (rc != CH_OK) return rc;
  a.mode = MODE_EVAL; a.maxit = 1; a.alpha[0] = 0.0; a.hist_slot[0] = x_slot; a.cand_slot = cand_slot; a.active = nullptr; a.abstol = 1e-6; a.reltol = 1e-3;
  a.dumpA = dumpG; a.dumpC = dumpC; a.dumpF = dumpF; a.dumpQ = dumpQ && c->nwt.path != 2 ? dumpQ : c->ac.d_dumpQ.p; a.dump_stride = ds;
  Summary sm;
  rc = c->run_newton(a, nullptr, sm, lds_extra);
  if (rc != CH_OK) return rc;
  // (sparse path: the charges of the evaluation are one vector per sample, which IS the dense layout of its single block)
  if (c->nwt.path == 2 && dumpQ && hipMemcpyAsync(dumpQ, c->sp.Q.p, (size_t)S * c->desc.A.n_unk * sizeof(double), hipMemcpyDeviceToDevice, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  if (c->nwt.path == 2) {   // the sparse evaluation left G (alpha0 = 0), C and F in CSR / vector form: expand to the dense blocks
    const int n = c->desc.A.n_unk, nnz = (int)c->sp.h_colidx.size();
    hipLaunchKernelGGL(csr_to_dense_kernel, dim3((n + 63) / 64, S), dim3(64), 0, c->ctx->stream, (const int*)c->sp.rowptr.p, (const int*)c->sp.colidx.p,
                       (const double*)c->sp.Aval.p, (const double*)c->sp.Cval.p, (const double*)c->sp.F.p, n, nnz, S, dumpG, dumpC, dumpF, dumpC ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return CH_ERR_DEVICE;
  }
  return CH_OK;
}

// Before the DC solve: the tables are brought up to date, and a coupled system too large for the dense LU (`lu`: what the message
// calls it) is refused
static int smallsignal_prepare(ch_circuit* c, const std::string& who, const char* lu) {
  const int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  if (c->nwt.path == 2 && c->desc.A.n_unk > 4096) { c->set_err(who + ": the coupled system has more than 4096 unknowns (" + lu + ")"); return CH_ERR_UNSUPPORTED; }
  return CH_OK;
}

// After the DC solve (operating point in slot 0): G, C and F(src) there as per-block dense dumps; d_dumpA and d_dumpQ are scratch
static int smallsignal_linearise(ch_circuit* c, int mode) {
  const int nblk = c->ac_ncomp() * c->tab.S, ds = c->ac_ds();
  const size_t nA = (size_t)nblk * ds * ds, nF = (size_t)nblk * ds;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(c->ac.d_dumpG.alloc(nA)); HIPCHK(c->ac.d_dumpC.alloc(nA)); HIPCHK(c->ac.d_dumpA.alloc(nA)); HIPCHK(c->ac.d_dumpF0.alloc(nF)); HIPCHK(c->ac.d_dumpQ.alloc(nF));
  return smallsignal_eval(c, c->nwt.base, c->own_sources(), 0, mode, c->ac.d_dumpF0.p, c->ac.d_dumpG.p, c->ac.d_dumpC.p);
}

static int check_frequencies(ch_circuit* c, int n_freq, const double* freqs_hz) {
  for (int i = 0; i < n_freq; ++i) if (!(freqs_hz[i] >= 0.0) || !std::isfinite(freqs_hz[i])) { c->set_err("frequencies must be finite and non-negative"); return CH_ERR_INVALID; }
  return CH_OK;
}

// (checked frequencies) -> rad/s on the device; the failure flag of the complex solves starts at 0
static int upload_omega(ch_circuit* c, int n_freq, const double* freqs_hz) {
  std::vector<double> w(n_freq);
  for (int i = 0; i < n_freq; ++i) w[i] = 6.283185307179586 * freqs_hz[i];
  if (c->ac.d_omega.upload(w, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  std::vector<int> z(1, 0);
  if (c->ac.d_acfail.upload(z, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  return CH_OK;
}

// The timing bracket of every launcher that times itself: the circuit's two events around its launches.  timed_end waits for the
// stream and ADDS the milliseconds since timed_begin to *ms: launch_acsens_rhs and transens_point accumulate over their launches,
// the solve launchers (launch_sens, launch_freq_chunks) are handed a field that is zero and are called once per field.
static hipError_t timed_begin(ch_circuit* c) { return hipEventRecord(c->nwt.ev0, c->ctx->stream); }
static hipError_t timed_end(ch_circuit* c, float* ms) {
  hipStream_t st = c->ctx->stream;
  float t = 0.0f;
  hipError_t e = hipEventRecord(c->nwt.ev1, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipEventElapsedTime(&t, c->nwt.ev0, c->nwt.ev1);
  *ms += t;
  return e;
}

// doubles of dynamic LDS a launch of `kernel` may ask for beside its static share: what raise_lds_ceilings granted
static hipError_t lds_budget_doubles(const void* kernel, size_t* doubles) {
  hipFuncAttributes fa;
  const hipError_t e = hipFuncGetAttributes(&fa, kernel);
  if (e == hipSuccess) *doubles = (size_t)lds_dynamic_ceiling((int)fa.sharedSizeBytes) / sizeof(double);
  return e;
}

// ---- AC and noise ------------------------------------------------------------------------------
// The AC right-hand side b = -(F(src + ac) - F(src)), exact because every source enters F linearly: one more evaluation, after the
// residual alone, with the AC magnitudes added to the sources; b replaces F(src + ac) in d_dumpF
static int ac_rhs(ch_circuit* c, int mode) {
  const size_t nF = (size_t)c->ac_ncomp() * c->tab.S * c->ac_ds();
  if (c->ac.d_dumpF.alloc(nF) != hipSuccess) return CH_ERR_DEVICE;
  c->ac.scale = 1.0;
  const int rc = smallsignal_eval(c, c->nwt.base, c->own_sources(), 0, mode, c->ac.d_dumpF.p, c->ac.d_dumpA.p, nullptr);
  c->ac.scale = 0.0;
  if (rc != CH_OK) return rc;
  hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((nF + 255) / 256)), dim3(256), 0, c->ctx->stream, c->ac.d_dumpF.p, (const double*)c->ac.d_dumpF0.p, (long)nF);
  return CH_OK;
}

// Front half of ch_ac / ch_noise: DC operating point (a sample that fails refuses the call), the dense dumps and, for ch_ac, b
static int ac_linearise(ch_circuit* c, const ch_dc_opts* o, ch_stats* st, bool want_b) {
  int rc = smallsignal_prepare(c, "AC / noise analysis", "dense complex LU");
  if (rc != CH_OK) return rc;
  rc = c->dc_solve(*o, 0, nullptr, st);
  if (rc != CH_OK) return rc;
  const int mode = o->tran_mode ? 2 : 0;
  rc = smallsignal_linearise(c, mode);
  if (rc != CH_OK || !want_b) return rc;
  return ac_rhs(c, mode);
}

// (G + jwC) solves of one analysis: `ny` systems per frequency.  Up to 96 unknowns the complex LU of a system runs in one
// wavefront with its matrices in LDS; larger coupled systems (sparse path) take the 256-thread variant with a global
// workspace, a chunk of frequencies per launch so that the workspace stays below 1 GiB.
static int launch_ac(ch_circuit* c, AcArgs& a, int n_freq, int ny, int ds) {
  const size_t per = ac_system_doubles(ds);
  const bool contrib = a.noise && a.contrib_out;   // (ch_noise_ex with a contributions buffer: the sibling instantiations)
  if (ds <= 96) {
    a.work = nullptr; a.f0 = 0;
    if (contrib) hipLaunchKernelGGL((ac_block_kernel<64, true>), dim3(n_freq, ny), dim3(64), per * sizeof(double), c->ctx->stream, a);
    else hipLaunchKernelGGL(ac_block_kernel<64>, dim3(n_freq, ny), dim3(64), per * sizeof(double), c->ctx->stream, a);
    return hipGetLastError() == hipSuccess ? CH_OK : CH_ERR_DEVICE;
  }
  const int chunk = dense_work_chunk(per, ny, n_freq);
  ScopedWorkspace work;
  if (work.alloc((size_t)chunk * ny * per) != hipSuccess) { c->set_err("AC / noise analysis: out of device memory for the dense complex LU workspace"); return CH_ERR_DEVICE; }
  for (int f0 = 0; f0 < n_freq; f0 += chunk) {
    a.work = work.p; a.f0 = f0;
    if (contrib) hipLaunchKernelGGL((ac_block_kernel<256, true>), dim3(std::min(chunk, n_freq - f0), ny), dim3(256), 0, c->ctx->stream, a);
    else hipLaunchKernelGGL(ac_block_kernel<256>, dim3(std::min(chunk, n_freq - f0), ny), dim3(256), 0, c->ctx->stream, a);
    if (hipGetLastError() != hipSuccess) return CH_ERR_DEVICE;
  }
  return hipStreamSynchronize(c->ctx->stream) == hipSuccess ? CH_OK : CH_ERR_DEVICE;
}

// The plain AC solves (ch_ac, and the x of ch_ac_sens): (G + jwC) x = b for every (frequency, block, sample), into d_xac
// [S][n_freq][n_unk][2].  Wants ac_rhs and upload_omega done.
static int ac_solve(ch_circuit* c, const BlockMeta* bmeta, int n_freq) {
  const int S = c->tab.S, ds = c->ac_ds(), nu = c->desc.A.n_unk;
  if (c->ac.d_xac.alloc((size_t)S * n_freq * nu * 2) != hipSuccess) return CH_ERR_DEVICE;
  AcArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = bmeta; a.G = c->ac.d_dumpG.p; a.C = c->ac.d_dumpC.p; a.b = c->ac.d_dumpF.p; a.ds = ds; a.S = S; a.n_unk = nu; a.n_freq = n_freq; a.n_comp = c->ac_ncomp();
  a.omega = c->ac.d_omega.p; a.x_out = c->ac.d_xac.p; a.noise = 0; a.fail = c->ac.d_acfail.p;
  return launch_ac(c, a, n_freq, c->ac_ncomp() * S, ds);
}

// ch_ac in two halves.  ac_device_solve: the checks and every launch, x left in c->ac.d_xac in unknown order; ch_ac_impl reads it back
// and expands it, ch_ac_measure (ch_engine_fmeasure.hpp) measures it where it lies.  st and t0 carry the statistics across.
static int ac_device_solve(ch_circuit* c, const ch_dc_opts* o, int32_t n_freq, const double* freqs_hz, ch_stats& st, hclock::time_point& t0, ch_stats* stats) {
  int rc = check_frequencies(c, n_freq, freqs_hz);
  if (rc != CH_OK) return rc;
  t0 = hclock::now();
  std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  rc = ac_linearise(c, o, &st, true);
  st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (rc != CH_OK) { if (stats) *stats = st; return rc; }
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, nblk = c->ac_ncomp() * S, ds = c->ac_ds();
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  const BlockMeta* bmeta = c->ac_bmeta();
  if (!bmeta) return CH_ERR_DEVICE;
  if (env_on(Env::DEBUG_AC) && ds <= 8 && nblk == 1) {   // diagnostic: the linearisation the complex solves start from
    std::vector<double> hg((size_t)ds * ds), hc((size_t)ds * ds), hb(ds);
    (void)hipStreamSynchronize(c->ctx->stream);
    (void)hipMemcpy(hg.data(), c->ac.d_dumpG.p, hg.size() * sizeof(double), hipMemcpyDeviceToHost); (void)hipMemcpy(hc.data(), c->ac.d_dumpC.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(hb.data(), c->ac.d_dumpF.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost);
    { std::vector<double> hx(A.n_unk); (void)hipMemcpy(hx.data(), c->nwt.d_X.p, hx.size() * sizeof(double), hipMemcpyDeviceToHost);
      std::fprintf(stderr, "[ac] state:"); for (double v : hx) std::fprintf(stderr, " %.12e", v); std::fprintf(stderr, "\n"); }
    for (int i = 0; i < ds; ++i) { std::fprintf(stderr, "[ac] G row %d:", i); for (int j = 0; j < ds; ++j) std::fprintf(stderr, " %.9e", hg[(size_t)i * ds + j]); std::fprintf(stderr, " | C:"); for (int j = 0; j < ds; ++j) std::fprintf(stderr, " %.9e", hc[(size_t)i * ds + j]); std::fprintf(stderr, " | b %.9e\n", hb[i]); }
  }
  return ac_solve(c, bmeta, n_freq);
}
// second half of ch_ac, ch_ac_measure without slots and ch_noise: the statistics and the return code.  who: the analysis, for the
// message; own_launches: the call's kernels beside the Newton launches; fail: the failure flag of the complex solves (c->ac.d_acfail)
static int ac_finish(ch_circuit* c, const char* who, ch_stats& st, hclock::time_point t0, int n_freq, int own_launches, int fail, ch_stats* stats) {
  const int S = c->tab.S;
  st.n_kernel_launches = c->stats.n_launch + own_launches; st.nfactors += (int64_t)n_freq * S; st.nsolve += (int64_t)n_freq * S;
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (stats) *stats = st;
  if (fail) { c->set_err(std::string(who) + ": singular small-signal matrix G + jwC"); return CH_ERR_SINGULAR; }
  return CH_OK;
}

static int ch_ac_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_freq, const double* freqs_hz, double* x_ac_out, ch_stats* stats) {
  if (!c || !o || n_freq < 1 || !freqs_hz || !x_ac_out) return CH_ERR_INVALID;
  CallScope call(c);
  ch_stats st; hclock::time_point t0;
  const int rc = ac_device_solve(c, o, n_freq, freqs_hz, st, t0, stats);
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  const int S = c->tab.S;
  const size_t nx = (size_t)S * n_freq * A.n_unk * 2;
  std::vector<double> xs(nx);
  int fail = 0;
  if (hipMemcpyAsync(xs.data(), c->ac.d_xac.p, nx * sizeof(double), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipStreamSynchronize(c->ctx->stream) != hipSuccess) { c->set_err("AC solve failed on the device"); return CH_ERR_DEVICE; }
  for (size_t sf = 0; sf < (size_t)S * n_freq; ++sf) acsens_expand_mna(A, &xs[sf * A.n_unk * 2], x_ac_out + sf * A.n_mna * 2);   // unknown order -> MNA order
  return ac_finish(c, "AC analysis", st, t0, n_freq, 2, fail, stats);
}

// The observed unknown of a noise analysis: -1 for a node held by ideal sources (or ground); CH_ERR_INVALID with a message otherwise
static int noise_output_unknown(ch_circuit* c, int32_t out_kind, int32_t out_index, int& u_out) {
  const Analysis& A = c->desc.A;
  u_out = -1;
  if (out_kind == 0) { if (out_index < 0 || out_index > c->desc.n_nodes) { c->set_err("noise: output node out of range"); return CH_ERR_INVALID; } u_out = out_index == 0 ? -1 : A.node_unknown[out_index]; }
  else if (out_kind == 1) {
    if (out_index < 0 || out_index >= (int)c->desc.dev.size() || c->desc.dev[out_index].branch < 0) { c->set_err("noise: output device has no branch current"); return CH_ERR_INVALID; }
    u_out = A.branch_unknown[c->desc.dev[out_index].branch];
    if (u_out < 0) { c->set_err("noise: the output branch current was eliminated (observe it when building the circuit)"); return CH_ERR_INVALID; }
  } else return CH_ERR_INVALID;
  return CH_OK;
}

// Columns of the source table of block `comp`, in table order: a resistor owns one, a MOSFET two (thermal, flicker; their power
// is 0 in an analysis without MOSFET noise), a compiled module va::MAX_NOISE.  entry: index into the table; hdev: device of ch_desc
static void noise_columns(ch_circuit* c, int comp, std::vector<int>& entry, std::vector<int>& hdev) {
  entry.clear(); hdev.clear();
  const int dofs = c->ac_dofs(comp), ndev = c->ac_ndev(comp);
  for (int d = 0; d < ndev; ++d) {
    const EDev& e = c->desc.A.edev[dofs + d];
    const int n = e.kind == K_R ? 1 : (e.kind == K_MOS ? 2 : (e.kind == K_VA ? va::MAX_NOISE : 0));
    for (int k = 0; k < n; ++k) { entry.push_back(d * va::MAX_NOISE + k); hdev.push_back(e.hdev); }
  }
}

// The MOSFET noise-parameter table of one analysis, [MOS classes][CH_B4N_NPAR] (ch_noise_params.hpp), on the host
static int mos_noise_params(ch_circuit* c, std::vector<double>& table) {
  const int n_cls = c->tab.n_cls;
  std::vector<int> model_of(n_cls); std::vector<double> type_of(n_cls);
  for (int cl = 0; cl < n_cls; ++cl) {
    model_of[cl] = c->desc.dev[class_hdev(c->desc, c->tab, cl)].ipar[0];
    const double tp = c->desc.model[model_of[cl]][CH_B4_type];
    type_of[cl] = std::isnan(tp) ? 1.0 : tp;
  }
  std::string err;
  const int rc = b4n_table(model_of, type_of, c->ac.mos_noise_given, table, err);
  if (rc != CH_OK) c->set_err(err);   // (b4n_table's text says "model card <index>": NoiseSolution._failure of solution.py reads the index out of it to add the card's name)
  return rc;
}

// MOSFET noise of the output block: the per-class parameter table and the second table launch.  npar == nullptr (ch_noise_ex, and the
// operating point of ch_noise_sens): the table is built and uploaded here, the failure flag starts at 0 and the operand rows are
// kept, as is the table on the host (c->ac.mos_npar_host).  Otherwise (the perturbed and shifted tables of ch_noise_sens) the launch reads the class list, the columns and the
// parameter table it is given, keeps no operand rows and adds to the same failure flag.
static int launch_mos_noise(ch_circuit* c, const NoiseTabArgs& t, const int* dcls = nullptr, const double* mosp = nullptr, const double* npar = nullptr) {
  if (!npar) {
    std::vector<double>& table = c->ac.mos_npar_host;
    const int rc = mos_noise_params(c, table);
    if (rc != CH_OK) return rc;
    std::vector<int> z(1, 0);
    if (c->ac.d_mos_npar.upload(table, c->ctx->stream) != hipSuccess || c->ac.d_mos_fail.upload(z, c->ctx->stream) != hipSuccess ||
        c->ac.d_mos_op.alloc((size_t)t.S * t.ndev * B4NO_COUNT) != hipSuccess) return CH_ERR_DEVICE;
  }
  MosNoiseArgs m; std::memset(&m, 0, sizeof(m));
  m.dkind = t.dkind; m.dterm = t.dterm; m.dhdev = t.dhdev; m.dcls = dcls ? dcls : c->tab.d_dcls.p; m.dmult = t.dmult; m.temp_s = t.temp_s; m.mosp = mosp ? mosp : c->tab.d_mosp.p;
  m.npar = npar ? npar : c->ac.d_mos_npar.p;
  m.X = t.X; m.kv = t.kv; m.Spar = t.Spar; m.Stemp = t.Stemp; m.Ssrc = t.Ssrc; m.Smos = c->tab.Smos; m.nk = t.nk; m.S = t.S; m.n_unk = t.n_unk;
  m.dofs = t.dofs; m.ndev = t.ndev; m.uofs = t.uofs; m.nc = t.nc; m.na = t.na; m.nb = t.nb; m.pwr = t.pwr; m.ex = t.ex;
  m.operands = npar ? nullptr : c->ac.d_mos_op.p; m.fail = c->ac.d_mos_fail.p;
  hipLaunchKernelGGL(mos_noise_table_kernel, dim3((t.ndev * t.S + 63) / 64), dim3(64), 0, c->ctx->stream, m);
  return hipGetLastError() == hipSuccess ? CH_OK : CH_ERR_DEVICE;
}

// ---- shared by ch_noise / ch_noise_ex and ch_noise_sens (ch_engine_noisesens.hpp) ----
// The source table of block `comp` at the operating point (ring slot 0) with the circuit's own tables: its buffers, the known-node
// values on the device, the arguments of the table kernels; then the launches.
static int noise_table_setup(ch_circuit* c, int mode, int comp, int n_freq, NoiseTabArgs& t) {
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, ndev_b = c->ac_ndev(comp), n_tab = ndev_b * va::MAX_NOISE;
  if (c->ac.d_noise_a.alloc((size_t)S * n_tab) != hipSuccess || c->ac.d_noise_b.alloc((size_t)S * n_tab) != hipSuccess ||
      c->ac.d_noise_pwr.alloc((size_t)S * n_tab) != hipSuccess || c->ac.d_noise_exp.alloc((size_t)S * n_tab) != hipSuccess ||
      c->ac.d_psd.alloc((size_t)S * n_freq) != hipSuccess) return CH_ERR_DEVICE;
  NewtonArgs na0 = c->nwt.base;
  const int rc = c->set_sources(na0, 0.0, mode); if (rc != CH_OK) return rc;
  if (na0.inline_vals) {  // the table kernel reads the known-node values from the device buffer
    std::memcpy(c->nwt.h_stage, na0.vals_inline, (size_t)(na0.nk + na0.nsrc) * sizeof(double));
    if (hipMemcpyAsync(c->nwt.d_kv.p, c->nwt.h_stage, (size_t)(na0.nk + na0.nsrc) * sizeof(double), hipMemcpyHostToDevice, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  }
  std::memset(&t, 0, sizeof(t));
  t.dkind = c->stru.d_dkind.p; t.dterm = c->stru.d_dterm.p; t.dsrc = c->stru.d_dsrc.p; t.dcls_local = c->tab.d_dcls_local.p; t.dhdev = c->stru.d_dhdev.p;
  t.dpar = c->tab.d_dpar.p; t.dmult = c->tab.d_dmult.p; t.vapar = c->tab.d_vapar.p; t.va_stride = c->nwt.base.va_stride; t.temp_s = c->tab.d_temp.p; t.gmin_s = c->tab.d_gmin.p;
  t.X = c->nwt.d_X.p; t.kv = c->nwt.d_kv.p;  // slot 0 holds the operating point
  t.Spar = c->tab.Spar; t.Stemp = c->tab.Stemp; t.Sgmin = c->tab.Sgmin; t.Ssrc = c->tab.Ssrc; t.nk = (int)A.known.size(); t.S = S; t.n_unk = A.n_unk;
  t.dofs = c->ac_dofs(comp); t.ndev = ndev_b; t.uofs = c->ac_uofs(comp); t.nc = c->ac_nc(comp);
  t.na = c->ac.d_noise_a.p; t.nb = c->ac.d_noise_b.p; t.pwr = c->ac.d_noise_pwr.p; t.ex = c->ac.d_noise_exp.p;
  return CH_OK;
}
static int noise_table_launch(ch_circuit* c, const NoiseTabArgs& t, int mos_noise, const int* dcls = nullptr, const double* mosp = nullptr, const double* npar = nullptr) {
  hipLaunchKernelGGL(noise_table_kernel, dim3((t.ndev * t.S + 63) / 64), dim3(64), 0, c->ctx->stream, t);
  return mos_noise ? launch_mos_noise(c, t, dcls, mosp, npar) : (int)CH_OK;
}
// the adjoint solves of the output block over the table noise_table_setup named (contributions: the caller adds them)
static int noise_solve_args(ch_circuit* c, int comp, int u_out, int n_freq, AcArgs& a) {
  const int S = c->tab.S;
  std::memset(&a, 0, sizeof(a));
  a.bmeta = c->ac_bmeta(); a.G = c->ac.d_dumpG.p; a.C = c->ac.d_dumpC.p; a.b = nullptr; a.ds = c->ac_ds(); a.S = S; a.n_unk = c->desc.A.n_unk; a.n_freq = n_freq; a.n_comp = c->ac_ncomp();
  if (!a.bmeta) return CH_ERR_DEVICE;
  a.omega = c->ac.d_omega.p; a.noise = 1; a.comp_out = comp; a.row_out = u_out - c->ac_uofs(comp); a.n_noise = c->ac_ndev(comp) * va::MAX_NOISE;
  a.noise_a = c->ac.d_noise_a.p; a.noise_b = c->ac.d_noise_b.p; a.noise_pwr = c->ac.d_noise_pwr.p; a.noise_exp = c->ac.d_noise_exp.p;
  a.psd_out = c->ac.d_psd.p; a.fail = c->ac.d_acfail.p; a.contrib_out = nullptr; a.contrib_col = c->ac.d_contrib_col.p; a.n_col = 0;
  return CH_OK;
}

// ch_noise and ch_noise_ex: mos_noise = 0 and contrib_out = nullptr is ch_noise, launch for launch
static int noise_run(ch_circuit* c, const ch_dc_opts* o, int mos_noise, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out,
                     double* contrib_out, ch_stats* stats) {
  if (!c || !o || n_freq < 1 || !freqs_hz || !psd_out) return CH_ERR_INVALID;
  CallScope call(c);
  int rc = check_frequencies(c, n_freq, freqs_hz);
  if (rc != CH_OK) return rc;
  auto t0 = hclock::now();
  ch_stats st; std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  c->ac.last_noise.valid = false;
  const Analysis& A = c->desc.A;
  int u_out = -1;
  rc = noise_output_unknown(c, out_kind, out_index, u_out);
  if (rc != CH_OK) return rc;
  rc = ac_linearise(c, o, &st, false);
  st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (rc != CH_OK) { if (stats) *stats = st; return rc; }
  const int S = c->tab.S, ds = c->ac_ds();
  if (u_out < 0) {  // a node held by ideal sources carries no noise
    std::fill(psd_out, psd_out + (size_t)S * n_freq, 0.0);
    if (stats) *stats = st;
    return CH_OK;   // (no block, no source table: nothing is written to contrib_out, which has no columns)
  }
  const int comp = c->ac_comp_of(u_out);
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  // noise table of the output block at the operating point (device side)
  const int ndev_b = c->ac_ndev(comp), n_tab = ndev_b * va::MAX_NOISE;
  {
    NoiseTabArgs t;
    rc = noise_table_setup(c, o->tran_mode ? 2 : 0, comp, n_freq, t); if (rc != CH_OK) return rc;
    rc = noise_table_launch(c, t, mos_noise); if (rc != CH_OK) return rc;
  }
  // contributions: the kernel writes the table's columns alone, [S][n_freq][n_col], into a workspace of this call
  ScopedWorkspace contrib;
  size_t n_col = 0;
  if (contrib_out) {
    std::vector<int> col_entry, col_hdev, col_of(std::max(1, n_tab), -1);
    noise_columns(c, comp, col_entry, col_hdev);
    n_col = col_entry.size();
    for (size_t k = 0; k < n_col; ++k) col_of[col_entry[k]] = (int)k;
    if (c->ac.d_contrib_col.upload(col_of, c->ctx->stream) != hipSuccess || contrib.alloc(std::max<size_t>(1, (size_t)S * n_freq * n_col)) != hipSuccess) {
      c->set_err("noise analysis: out of device memory for the contributions"); return CH_ERR_DEVICE;
    }
  }
  AcArgs a;
  rc = noise_solve_args(c, comp, u_out, n_freq, a); if (rc != CH_OK) return rc;
  a.contrib_out = contrib_out ? contrib.p : nullptr; a.n_col = (int)n_col;
  { const int rc_l = launch_ac(c, a, n_freq, S, ds); if (rc_l != CH_OK) return rc_l; }
  int fail = 0;
  if (hipMemcpyAsync(psd_out, c->ac.d_psd.p, (size_t)S * n_freq * sizeof(double), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipStreamSynchronize(c->ctx->stream) != hipSuccess) { c->set_err("noise solve failed on the device"); return CH_ERR_DEVICE; }
  if (mos_noise || contrib_out) {   // ch_noise_ex proper: the source table (and the operand rows) come back for ch_noise_sources
    LastNoise& L = c->ac.last_noise;
    L.comp = comp; L.S = S; L.n_tab = n_tab; L.ndev = ndev_b; L.mos = mos_noise != 0;
    L.a.resize((size_t)S * n_tab); L.b.resize((size_t)S * n_tab); L.pwr.resize((size_t)S * n_tab); L.ex.resize((size_t)S * n_tab);
    L.op.assign((size_t)S * ndev_b * B4NO_COUNT, 0.0);
    int mfail = 0;
    bool okc = hipMemcpy(L.a.data(), c->ac.d_noise_a.p, L.a.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(L.b.data(), c->ac.d_noise_b.p, L.b.size() * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(L.pwr.data(), c->ac.d_noise_pwr.p, L.pwr.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
               hipMemcpy(L.ex.data(), c->ac.d_noise_exp.p, L.ex.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    if (okc && mos_noise) okc = hipMemcpy(L.op.data(), c->ac.d_mos_op.p, L.op.size() * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
                                hipMemcpy(&mfail, c->ac.d_mos_fail.p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
    if (okc && contrib_out && n_col) okc = hipMemcpy(contrib_out, contrib.p, (size_t)S * n_freq * n_col * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess;
    if (!okc) { c->set_err("noise analysis: reading the source table back failed"); return CH_ERR_DEVICE; }
    if (mfail) { c->set_err("MOSFET noise: a BSIM4 card without an intrinsic charge model (capmod 0 or xpart < 0) has no inversion charge to take the channel noise from"); return CH_ERR_UNSUPPORTED; }
    L.valid = true;
  }
  return ac_finish(c, "noise analysis", st, t0, n_freq, 1, fail, stats);
}

static int ch_noise_impl(ch_circuit* c, const ch_dc_opts* o, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out, ch_stats* stats) {
  return noise_run(c, o, 0, out_kind, out_index, n_freq, freqs_hz, psd_out, nullptr, stats);
}

static int ch_noise_ex_impl(ch_circuit* c, const ch_dc_opts* o, const ch_noise_opts* no, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz,
                            double* psd_out, double* contrib_out, ch_stats* stats) {
  if (!no) return CH_ERR_INVALID;
  return noise_run(c, o, no->mos_noise ? 1 : 0, out_kind, out_index, n_freq, freqs_hz, psd_out, contrib_out, stats);
}

static int ch_set_mos_noise_impl(ch_circuit* c, int32_t model, const double* par) {
  if (!c || !par) return CH_ERR_INVALID;
  if (model < 0 || model >= (int)c->desc.model.size()) { c->set_err("ch_set_mos_noise: model index out of range"); return CH_ERR_INVALID; }
  c->ac.mos_noise_given.resize(c->desc.model.size());
  c->ac.mos_noise_given[model].assign(par, par + CH_B4N_NPAR);
  return CH_OK;
}

// The source table of the output block.  Every array null: *n_src = the number of columns, a property of the structure (no
// analysis needed).  Otherwise the columns of the table the last ch_noise_ex built for this output block, sample `sample`.
static int ch_noise_sources_impl(ch_circuit* c, int32_t out_kind, int32_t out_index, int32_t sample, int32_t* n_src, int32_t* dev, int32_t* ta, int32_t* tb, double* pwr,
                                 double* ex, double* mos_operands) {
  if (!c || !n_src) return CH_ERR_INVALID;
  CallScope call(c);
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  int u_out = -1;
  rc = noise_output_unknown(c, out_kind, out_index, u_out);
  if (rc != CH_OK) return rc;
  *n_src = 0;
  if (u_out < 0) return CH_OK;
  const int comp = c->ac_comp_of(u_out), uofs = c->ac_uofs(comp);
  std::vector<int> entry, hdev;
  noise_columns(c, comp, entry, hdev);
  *n_src = (int32_t)entry.size();
  if (!dev && !ta && !tb && !pwr && !ex && !mos_operands) return CH_OK;
  const LastNoise& L = c->ac.last_noise;
  if (!L.valid || L.comp != comp || L.n_tab != c->ac_ndev(comp) * va::MAX_NOISE) { c->set_err("ch_noise_sources: no ch_noise_ex has built the source table of this output"); return CH_ERR_INVALID; }
  if (sample < 0 || sample >= L.S) { c->set_err("ch_noise_sources: sample out of range"); return CH_ERR_INVALID; }
  const Analysis& A = c->desc.A;
  auto mna = [&](int local) { return local < 0 ? -1 : A.unk_mna[uofs + local]; };
  for (size_t k = 0; k < entry.size(); ++k) {
    const size_t e = (size_t)sample * L.n_tab + entry[k];
    if (dev) dev[k] = hdev[k];
    if (ta) ta[k] = mna(L.a[e]);
    if (tb) tb[k] = mna(L.b[e]);
    if (pwr) pwr[k] = L.pwr[e];
    if (ex) ex[k] = L.ex[e];
    if (mos_operands) {
      const int d = entry[k] / va::MAX_NOISE;
      for (int q = 0; q < B4NO_COUNT; ++q) mos_operands[k * B4NO_COUNT + q] = L.op[((size_t)sample * L.ndev + d) * B4NO_COUNT + q];
    }
  }
  return CH_OK;
}
