// ch_engine_ac.hpp — small-signal analyses (AC, noise): linearisation at the operating point, the dense complex solves
// (ac_block_kernel) and the two entry-point bodies.  Included by ch_engine.hip behind the definition of ch_circuit.
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

// ---- small-signal analyses -------------------------------------------------------------------
// One MODE_EVAL launch at the operating point (slot 0): pass 0 leaves G, C and F(src) as dense dumps, pass 1 F(src + ac) for the
// AC right-hand side
static int ac_eval_pass(ch_circuit* c, int mode, int pass) {
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, ds = c->ac_ds();
  NewtonArgs a = c->nwt.base;
  c->ac.scale = pass == 0 ? 0.0 : 1.0;
  int rc = c->set_sources(a, 0.0, mode);
  c->ac.scale = 0.0;
  if (rc != CH_OK) return rc;
  a.mode = MODE_EVAL; a.maxit = 1; a.alpha[0] = 0.0; a.hist_slot[0] = 0; a.cand_slot = 1; a.active = nullptr; a.abstol = 1e-6; a.reltol = 1e-3;
  a.dumpA = pass == 0 ? c->ac.d_dumpG.p : c->ac.d_dumpA.p; a.dumpC = pass == 0 ? c->ac.d_dumpC.p : nullptr;
  a.dumpF = pass == 0 ? c->ac.d_dumpF0.p : c->ac.d_dumpF.p; a.dumpQ = c->ac.d_dumpQ.p; a.dump_stride = ds;
  Summary sm;
  rc = c->run_newton(a, nullptr, sm);
  if (rc != CH_OK) return rc;
  if (c->nwt.path == 2) {   // the sparse evaluation left G (alpha0 = 0), C and F in CSR / vector form: expand to the dense blocks
    const int n = A.n_unk, nnz = (int)c->sp.h_colidx.size();
    hipLaunchKernelGGL(csr_to_dense_kernel, dim3((n + 63) / 64, S), dim3(64), 0, c->ctx->stream, (const int*)c->sp.rowptr.p, (const int*)c->sp.colidx.p,
                       (const double*)c->sp.Aval.p, (const double*)c->sp.Cval.p, (const double*)c->sp.F.p, n, nnz, S, c->ac.d_dumpG.p, c->ac.d_dumpC.p,
                       pass == 0 ? c->ac.d_dumpF0.p : c->ac.d_dumpF.p, pass == 0 ? 1 : 0);
  }
  return CH_OK;
}

// Shared front half of ch_ac / ch_noise: DC operating point (slot 0), then G, C (and the AC right-hand
// side b = -(F(src + ac) - F(src)), exact because every source enters F linearly) as per-block dense dumps.
static int ac_linearise(ch_circuit* c, const ch_dc_opts* o, ch_stats* st, bool want_b) {
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  if (c->nwt.path == 2 && c->desc.A.n_unk > 4096) { c->set_err("AC / noise analysis: the coupled system has more than 4096 unknowns (dense complex LU)"); return CH_ERR_UNSUPPORTED; }
  g_arena = &c->arena;
  rc = c->dc_solve(*o, 0, nullptr, st);
  if (rc != CH_OK) return rc;
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, nblk = c->ac_ncomp() * S, ds = c->ac_ds();
  const size_t nA = (size_t)nblk * ds * ds, nF = (size_t)nblk * ds;
  if (c->ac.d_dumpG.alloc(nA) != hipSuccess || c->ac.d_dumpC.alloc(nA) != hipSuccess || c->ac.d_dumpF0.alloc(nF) != hipSuccess ||
      c->ac.d_dumpF.alloc(nF) != hipSuccess || c->ac.d_dumpQ.alloc(nF) != hipSuccess || c->ac.d_dumpA.alloc(nA) != hipSuccess) return CH_ERR_DEVICE;
  const int mode = o->tran_mode ? 2 : 0;
  for (int pass = 0; pass < (want_b ? 2 : 1); ++pass) { rc = ac_eval_pass(c, mode, pass); if (rc != CH_OK) return rc; }
  if (want_b) {  // b = F0 - F1 (device side, in place in d_dumpF)
    hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((nF + 255) / 256)), dim3(256), 0, c->ctx->stream, c->ac.d_dumpF.p, (const double*)c->ac.d_dumpF0.p, (long)nF);
  }
  return CH_OK;
}

// (G + jwC) solves of one analysis: `ny` systems per frequency.  Up to 96 unknowns the complex LU of a system runs in one
// wavefront with its matrices in LDS; larger coupled systems (sparse path) take the 256-thread variant with a global
// workspace, a chunk of frequencies per launch so that the workspace stays below 1 GiB.
static int launch_ac(ch_circuit* c, AcArgs& a, int n_freq, int ny, int ds) {
  const size_t per = (size_t)2 * ds * (ds + 1);
  if (ds <= 96) {
    const size_t lds = per * sizeof(double);
    a.work = nullptr; a.f0 = 0;
    hipLaunchKernelGGL(ac_block_kernel<64>, dim3(n_freq, ny), dim3(64), lds, c->ctx->stream, a);
    return hipGetLastError() == hipSuccess ? CH_OK : CH_ERR_DEVICE;
  }
  const size_t cap = (size_t)1 << 27;   // doubles
  const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_freq, cap / (per * (size_t)ny)));
  double* work = nullptr;
  if (hipMalloc((void**)&work, (size_t)chunk * ny * per * sizeof(double)) != hipSuccess) { c->set_err("AC / noise analysis: out of device memory for the dense complex LU workspace"); return CH_ERR_DEVICE; }
  int rc = CH_OK;
  for (int f0 = 0; f0 < n_freq && rc == CH_OK; f0 += chunk) {
    a.work = work; a.f0 = f0;
    hipLaunchKernelGGL(ac_block_kernel<256>, dim3(std::min(chunk, n_freq - f0), ny), dim3(256), 0, c->ctx->stream, a);
    if (hipGetLastError() != hipSuccess) rc = CH_ERR_DEVICE;
  }
  if (hipStreamSynchronize(c->ctx->stream) != hipSuccess) rc = CH_ERR_DEVICE;
  (void)hipFree(work);
  return rc;
}

static int upload_omega(ch_circuit* c, int n_freq, const double* freqs_hz) {
  std::vector<double> w(n_freq);
  for (int i = 0; i < n_freq; ++i) { if (!(freqs_hz[i] >= 0.0) || !std::isfinite(freqs_hz[i])) { c->set_err("frequencies must be finite and non-negative"); return CH_ERR_INVALID; } w[i] = 6.283185307179586 * freqs_hz[i]; }
  if (c->ac.d_omega.upload(w, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  std::vector<int> z(1, 0);
  if (c->ac.d_acfail.upload(z, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
  return CH_OK;
}

static int ch_ac_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_freq, const double* freqs_hz, double* x_ac_out, ch_stats* stats) {
  if (!c || !o || n_freq < 1 || !freqs_hz || !x_ac_out) return CH_ERR_INVALID;
  CallScope call(c);
  auto t0 = hclock::now();
  ch_stats st; std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  int rc = ac_linearise(c, o, &st, true);
  st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (rc != CH_OK) { if (stats) *stats = st; return rc; }
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, nblk = c->ac_ncomp() * S, ds = c->ac_ds();
  g_arena = &c->arena;
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  const size_t nx = (size_t)S * n_freq * A.n_unk * 2;
  if (c->ac.d_xac.alloc(nx) != hipSuccess) return CH_ERR_DEVICE;
  AcArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = c->ac_bmeta(); a.G = c->ac.d_dumpG.p; a.C = c->ac.d_dumpC.p; a.b = c->ac.d_dumpF.p; a.ds = ds; a.S = S; a.n_unk = A.n_unk; a.n_freq = n_freq; a.n_comp = c->ac_ncomp();
  if (!a.bmeta) return CH_ERR_DEVICE;
  a.omega = c->ac.d_omega.p; a.x_out = c->ac.d_xac.p; a.noise = 0; a.fail = c->ac.d_acfail.p;
  if (env_on(Env::DEBUG_AC) && ds <= 8 && nblk == 1) {   // diagnostic: the linearisation the complex solves start from
    std::vector<double> hg((size_t)ds * ds), hc((size_t)ds * ds), hb(ds);
    (void)hipStreamSynchronize(c->ctx->stream);
    (void)hipMemcpy(hg.data(), c->ac.d_dumpG.p, hg.size() * sizeof(double), hipMemcpyDeviceToHost); (void)hipMemcpy(hc.data(), c->ac.d_dumpC.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipMemcpy(hb.data(), c->ac.d_dumpF.p, hb.size() * sizeof(double), hipMemcpyDeviceToHost);
    { std::vector<double> hx(A.n_unk); (void)hipMemcpy(hx.data(), c->nwt.d_X.p, hx.size() * sizeof(double), hipMemcpyDeviceToHost);
      std::fprintf(stderr, "[ac] state:"); for (double v : hx) std::fprintf(stderr, " %.12e", v); std::fprintf(stderr, "\n"); }
    for (int i = 0; i < ds; ++i) { std::fprintf(stderr, "[ac] G row %d:", i); for (int j = 0; j < ds; ++j) std::fprintf(stderr, " %.9e", hg[(size_t)i * ds + j]); std::fprintf(stderr, " | C:"); for (int j = 0; j < ds; ++j) std::fprintf(stderr, " %.9e", hc[(size_t)i * ds + j]); std::fprintf(stderr, " | b %.9e\n", hb[i]); }
  }
  rc = launch_ac(c, a, n_freq, nblk, ds);
  if (rc != CH_OK) return rc;
  std::vector<double> xs(nx);
  int fail = 0;
  if (hipMemcpyAsync(xs.data(), c->ac.d_xac.p, nx * sizeof(double), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipStreamSynchronize(c->ctx->stream) != hipSuccess) { c->set_err("AC solve failed on the device"); return CH_ERR_DEVICE; }
  st.n_kernel_launches = c->stats.n_launch + 2; st.nfactors += (int64_t)n_freq * S; st.nsolve += (int64_t)n_freq * S;
  // unknown space -> MNA order (known nodes carry no small signal: AC-driven sources are never eliminated)
  const int n_nodes = c->desc.n_nodes, nm = A.n_mna;
  for (int s = 0; s < S; ++s) for (int f = 0; f < n_freq; ++f) {
    const double* xu = &xs[(((size_t)s * n_freq + f) * A.n_unk) * 2];
    double* xo = x_ac_out + (((size_t)s * n_freq + f) * nm) * 2;
    for (int n = 1; n <= n_nodes; ++n) { const int u = A.node_unknown[n]; xo[2 * (n - 1)] = u >= 0 ? xu[2 * u] : 0.0; xo[2 * (n - 1) + 1] = u >= 0 ? xu[2 * u + 1] : 0.0; }
    for (int b = 0; b < A.n_branch; ++b) { const int u = A.branch_unknown[b]; xo[2 * (n_nodes + b)] = u >= 0 ? xu[2 * u] : CH_NAN; xo[2 * (n_nodes + b) + 1] = u >= 0 ? xu[2 * u + 1] : CH_NAN; }
  }
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (stats) *stats = st;
  if (fail) { c->set_err("AC analysis: singular small-signal matrix G + jwC"); return CH_ERR_SINGULAR; }
  return CH_OK;
}

static int ch_noise_impl(ch_circuit* c, const ch_dc_opts* o, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz, double* psd_out, ch_stats* stats) {
  if (!c || !o || n_freq < 1 || !freqs_hz || !psd_out) return CH_ERR_INVALID;
  CallScope call(c);
  auto t0 = hclock::now();
  ch_stats st; std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  const Analysis& A = c->desc.A;
  int u_out = -1;
  if (out_kind == 0) { if (out_index < 0 || out_index > c->desc.n_nodes) { c->set_err("noise: output node out of range"); return CH_ERR_INVALID; } u_out = out_index == 0 ? -1 : A.node_unknown[out_index]; }
  else if (out_kind == 1) {
    if (out_index < 0 || out_index >= (int)c->desc.dev.size() || c->desc.dev[out_index].branch < 0) { c->set_err("noise: output device has no branch current"); return CH_ERR_INVALID; }
    u_out = A.branch_unknown[c->desc.dev[out_index].branch];
    if (u_out < 0) { c->set_err("noise: the output branch current was eliminated (observe it when building the circuit)"); return CH_ERR_INVALID; }
  } else return CH_ERR_INVALID;
  int rc = ac_linearise(c, o, &st, false);
  st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (rc != CH_OK) { if (stats) *stats = st; return rc; }
  const int S = c->tab.S, ds = c->ac_ds();
  if (u_out < 0) {  // a node held by ideal sources carries no noise
    std::fill(psd_out, psd_out + (size_t)S * n_freq, 0.0);
    if (stats) *stats = st;
    return CH_OK;
  }
  const int comp = c->ac_comp_of(u_out);
  const int uofs = c->ac_uofs(comp), ncb = c->ac_nc(comp);
  g_arena = &c->arena;
  rc = upload_omega(c, n_freq, freqs_hz); if (rc != CH_OK) return rc;
  // noise table of the output block at the operating point (device side)
  const int ndev_b = c->ac_ndev(comp), n_tab = ndev_b * va::MAX_NOISE;
  if (c->ac.d_noise_a.alloc((size_t)S * n_tab) != hipSuccess || c->ac.d_noise_b.alloc((size_t)S * n_tab) != hipSuccess ||
      c->ac.d_noise_pwr.alloc((size_t)S * n_tab) != hipSuccess || c->ac.d_noise_exp.alloc((size_t)S * n_tab) != hipSuccess ||
      c->ac.d_psd.alloc((size_t)S * n_freq) != hipSuccess) return CH_ERR_DEVICE;
  {
    NewtonArgs na0 = c->nwt.base;
    rc = c->set_sources(na0, 0.0, o->tran_mode ? 2 : 0); if (rc != CH_OK) return rc;
    if (na0.inline_vals) {  // the table kernel reads the known-node values from the device buffer
      std::memcpy(c->nwt.h_stage, na0.vals_inline, (size_t)(na0.nk + na0.nsrc) * sizeof(double));
      if (hipMemcpyAsync(c->nwt.d_kv.p, c->nwt.h_stage, (size_t)(na0.nk + na0.nsrc) * sizeof(double), hipMemcpyHostToDevice, c->ctx->stream) != hipSuccess) return CH_ERR_DEVICE;
    }
    NoiseTabArgs t; std::memset(&t, 0, sizeof(t));
    t.dkind = c->stru.d_dkind.p; t.dterm = c->stru.d_dterm.p; t.dsrc = c->stru.d_dsrc.p; t.dcls_local = c->tab.d_dcls_local.p; t.dhdev = c->stru.d_dhdev.p;
    t.dpar = c->tab.d_dpar.p; t.dmult = c->tab.d_dmult.p; t.vapar = c->tab.d_vapar.p; t.va_stride = c->nwt.base.va_stride; t.temp_s = c->tab.d_temp.p; t.gmin_s = c->tab.d_gmin.p;
    t.X = c->nwt.d_X.p; t.kv = c->nwt.d_kv.p;  // slot 0 holds the operating point
    t.Spar = c->tab.Spar; t.Stemp = c->tab.Stemp; t.Sgmin = c->tab.Sgmin; t.Ssrc = c->tab.Ssrc; t.nk = (int)A.known.size(); t.S = S; t.n_unk = A.n_unk;
    t.dofs = c->ac_dofs(comp); t.ndev = ndev_b; t.uofs = uofs; t.nc = ncb;
    t.na = c->ac.d_noise_a.p; t.nb = c->ac.d_noise_b.p; t.pwr = c->ac.d_noise_pwr.p; t.ex = c->ac.d_noise_exp.p;
    hipLaunchKernelGGL(noise_table_kernel, dim3((ndev_b * S + 63) / 64), dim3(64), 0, c->ctx->stream, t);
  }
  AcArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = c->ac_bmeta(); a.G = c->ac.d_dumpG.p; a.C = c->ac.d_dumpC.p; a.b = nullptr; a.ds = ds; a.S = S; a.n_unk = A.n_unk; a.n_freq = n_freq; a.n_comp = c->ac_ncomp();
  if (!a.bmeta) return CH_ERR_DEVICE;
  a.omega = c->ac.d_omega.p; a.noise = 1; a.comp_out = comp; a.row_out = u_out - uofs; a.n_noise = n_tab;
  a.noise_a = c->ac.d_noise_a.p; a.noise_b = c->ac.d_noise_b.p; a.noise_pwr = c->ac.d_noise_pwr.p; a.noise_exp = c->ac.d_noise_exp.p;
  a.psd_out = c->ac.d_psd.p; a.fail = c->ac.d_acfail.p;
  { const int rc_l = launch_ac(c, a, n_freq, S, ds); if (rc_l != CH_OK) return rc_l; }
  int fail = 0;
  if (hipMemcpyAsync(psd_out, c->ac.d_psd.p, (size_t)S * n_freq * sizeof(double), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&fail, c->ac.d_acfail.p, sizeof(int), hipMemcpyDeviceToHost, c->ctx->stream) != hipSuccess ||
      hipStreamSynchronize(c->ctx->stream) != hipSuccess) { c->set_err("noise solve failed on the device"); return CH_ERR_DEVICE; }
  st.n_kernel_launches = c->stats.n_launch + 1; st.nfactors += (int64_t)n_freq * S; st.nsolve += (int64_t)n_freq * S;
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  if (stats) *stats = st;
  if (fail) { c->set_err("noise analysis: singular small-signal matrix G + jwC"); return CH_ERR_SINGULAR; }
  return CH_OK;
}
