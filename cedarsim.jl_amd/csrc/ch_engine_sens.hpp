// ch_engine_sens.hpp — DC parameter sensitivities by the direct method (ch_dc_sens): F(x, p) = 0  =>  G · dx/dp_k = -dF/dp_k at x*.
// The operating point and G come from the linearisation the small-signal analyses use (slot 0 of the state ring, a MODE_EVAL dump);
// dF/dp_k is a difference of two more MODE_EVAL launches in which ONLY the table the slot reaches is replaced by a perturbed copy
// (NewtonArgs carries the tables as pointers; the copies come from perturb_tables, ch_param_tables.hpp, out of the host tables
// finalize_params kept): no finalize_params rebuild, no second Newton solve, no read-back, and the circuit's own tables are never
// written.  The step rule and the MNA expansion are HIP-free (ch_sens_host.hpp); the solves run in sens_block_kernel.
// Included by ch_engine.hip behind ch_engine_ac.hpp.
#pragma once

extern "C++" {   // (included inside the extern "C" block of ch_engine.hip; templates need C++ linkage)

// one MODE_EVAL launch at the operating point (ring slot 0) with the tables of `a`, the source tables `src` and lds_extra bytes of
// dynamic LDS on top of the circuit's; F lands in dumpF as dense per-block vectors
static int sens_eval(ch_circuit* c, NewtonArgs a, SourceTables src, size_t lds_extra, int mode, double* dumpF, bool fill_g) {
  const int S = c->tab.S, ds = c->ac_ds();
  int rc = c->set_sources(a, 0.0, mode, src);
  if (rc != CH_OK) return rc;
  a.mode = MODE_EVAL; a.maxit = 1; a.alpha[0] = 0.0; a.hist_slot[0] = 0; a.cand_slot = 1; a.active = nullptr; a.abstol = 1e-6; a.reltol = 1e-3;
  a.dumpA = fill_g ? c->ac.d_dumpG.p : c->ac.d_dumpA.p; a.dumpC = fill_g ? c->ac.d_dumpC.p : nullptr; a.dumpF = dumpF; a.dumpQ = c->ac.d_dumpQ.p; a.dump_stride = ds;
  Summary sm;
  rc = c->run_newton(a, nullptr, sm, lds_extra);
  if (rc != CH_OK) return rc;
  if (c->nwt.path == 2) {
    const int n = c->desc.A.n_unk, nnz = (int)c->sp.h_colidx.size();
    hipLaunchKernelGGL(csr_to_dense_kernel, dim3((n + 63) / 64, S), dim3(64), 0, c->ctx->stream, (const int*)c->sp.rowptr.p, (const int*)c->sp.colidx.p,
                       (const double*)c->sp.Aval.p, (const double*)c->sp.Cval.p, (const double*)c->sp.F.p, n, nnz, S, c->ac.d_dumpG.p, c->ac.d_dumpC.p, dumpF, fill_g ? 1 : 0);
    if (hipGetLastError() != hipSuccess) return CH_ERR_DEVICE;
  }
  return CH_OK;
}

// The tables of one perturbed evaluation: slot `id` takes val[s] in sample s, everything else stays.  perturb_tables
// (ch_param_tables.hpp) makes the copies from the circuit's retained host tables; they go into the scratch buffers c->sens and `a`
// points at them.  The source tables stay on the host, in `o`.
static int sens_perturb(ch_circuit* c, int id, const std::vector<double>& val, TableOverride& o, NewtonArgs& a) {
  hipStream_t st = c->ctx->stream; Sensitivity& d = c->sens;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  const int rc = perturb_tables(c->desc, c->slots(), c->tab, id, val, o, c->err(), c->nwt.path == 1);
  if (rc != CH_OK) return rc;
  if (!o.dpar.empty()) { HIPCHK(d.d_dpar.upload(o.dpar, st)); a.dpar = d.d_dpar.p; }
  if (!o.dmult.empty()) { HIPCHK(d.d_dmult.upload(o.dmult, st)); a.dmult = d.d_dmult.p; }
  if (!o.gmin.empty()) { HIPCHK(d.d_gmin.upload(o.gmin, st)); a.gmin_s = d.d_gmin.p; }
  if (!o.temp.empty()) { HIPCHK(d.d_temp.upload(o.temp, st)); a.temp_s = d.d_temp.p; }
  if (!o.vapar.empty()) { HIPCHK(d.d_vapar.upload(o.vapar, st)); a.vapar = d.d_vapar.p; }
  if (!o.mosp.empty()) { HIPCHK(d.d_mosp.upload(o.mosp, st)); a.mosp = d.d_mosp.p; }
  if (!o.dcls.empty()) { HIPCHK(d.d_dcls.upload(o.dcls, st)); a.dcls = d.d_dcls.p; }
  if (!o.bmeta.empty()) {
    HIPCHK(d.d_bmeta.upload(o.bmeta, st)); HIPCHK(d.d_dcls_local.upload(o.dcls_local, st)); HIPCHK(d.d_mc_list.upload(o.mc_list, st));
    a.bmeta = d.d_bmeta.p; a.dcls_local = d.d_dcls_local.p; a.mc_list = d.d_mc_list.p;
  }
  a.mos_cols = o.mos_cols; a.n_mos_cls = o.n_mos_cls; a.max_mc = o.max_mc;
  if (o.va_setup && c->stru.n_va_inst > 0) {
    const int rcv = c->launch_va_setup(a.vapar, a.temp_s, d.d_vacache);
    if (rcv != CH_OK) return rcv;
    a.vacache = d.d_vacache.p;
  }
  return CH_OK;
}

// G · X = B for every (block, sample) and the columns k0 .. k0+kc of the right-hand sides, in chunks that fit
static int launch_sens(ch_circuit* c, SensArgs& a, int nblk, int n_par, size_t nF, float* ms_out, int* n_chunks, int* n_launches) {
  *n_chunks = 0; *n_launches = 0;
  const int ds = a.ds;
  hipStream_t st = c->ctx->stream;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(hipEventRecord(c->nwt.ev0, st));
  if (ds <= 96) {
    const size_t budget = (size_t)2 * 96 * 97;   // doubles: the ceiling ch_create raises for ac_block_kernel<64> as well
    const int kmax = std::max(1, sens_lds_columns(ds, budget));
    for (int k0 = 0; k0 < n_par; k0 += kmax) {
      SensArgs b = a;
      b.k0 = k0; b.kc = std::min(kmax, n_par - k0); b.blk0 = 0; b.work = nullptr;
      b.Fp = a.Fp + (size_t)k0 * nF; b.Fm = a.Fm + (size_t)k0 * nF; b.den = a.den + (size_t)k0 * a.S;
      const size_t lds = (size_t)ds * sens_lda(ds, b.kc) * sizeof(double);
      hipLaunchKernelGGL(sens_block_kernel<64>, dim3(nblk), dim3(64), lds, st, b);
      HIPCHK(hipGetLastError());
      *n_launches += 1; *n_chunks += 1;
    }
  } else {
    const int kmax = std::min(n_par, 32);
    const size_t per = (size_t)ds * sens_lda(ds, kmax), cap = (size_t)1 << 27;   // doubles
    const int bchunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nblk, cap / per));
    double* work = nullptr;
    if (hipMalloc((void**)&work, (size_t)bchunk * per * sizeof(double)) != hipSuccess) { c->set_err("ch_dc_sens: out of device memory for the dense LU workspace"); return CH_ERR_DEVICE; }
    int rc = CH_OK;
    for (int k0 = 0; k0 < n_par && rc == CH_OK; k0 += kmax) for (int b0 = 0; b0 < nblk && rc == CH_OK; b0 += bchunk) {
      SensArgs b = a;
      b.k0 = k0; b.kc = std::min(kmax, n_par - k0); b.blk0 = b0; b.work = work;
      b.Fp = a.Fp + (size_t)k0 * nF; b.Fm = a.Fm + (size_t)k0 * nF; b.den = a.den + (size_t)k0 * a.S;
      hipLaunchKernelGGL(sens_block_kernel<256>, dim3(std::min(bchunk, nblk - b0)), dim3(256), 0, st, b);
      if (hipGetLastError() != hipSuccess) rc = CH_ERR_DEVICE;
      *n_launches += 1; if (b0 == 0) *n_chunks += 1;
    }
    if (hipStreamSynchronize(st) != hipSuccess) rc = CH_ERR_DEVICE;
    (void)hipFree(work);
    if (rc != CH_OK) { c->set_err("ch_dc_sens: the dense solve failed on the device"); return rc; }
  }
  HIPCHK(hipEventRecord(c->nwt.ev1, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipEventElapsedTime(ms_out, c->nwt.ev0, c->nwt.ev1));
  return CH_OK;
}

static int ch_dc_sens_impl(ch_circuit* c, const ch_dc_opts* o, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* so, double* x_out, double* sens_out,
                           int32_t* status_out, ch_stats* stats) {
  if (!c || !o) return CH_ERR_INVALID;
  CallScope call(c);
  if (n_par < 1 || !slot_ids || !sens_out) { c->set_err("ch_dc_sens: at least one parameter slot and an output array"); return CH_ERR_INVALID; }
  for (int k = 0; k < n_par; ++k) if (slot_ids[k] < 0 || slot_ids[k] >= (int)c->desc.slot_kind.size()) { c->set_err("ch_dc_sens: slot id out of range"); return CH_ERR_INVALID; }
  ch_sens_opts sopt; ch_sens_opts_default(&sopt);
  if (so) sopt = *so;
  if (!(sopt.rel_step > 0.0) || !std::isfinite(sopt.rel_step)) { c->set_err("ch_dc_sens: rel_step must be positive and finite"); return CH_ERR_INVALID; }
  auto t0 = hclock::now();
  ch_stats st; std::memset(&st, 0, sizeof(st));
  c->stats.reset();
  // ---- operating point (slot 0); a sample that fails keeps its status, the others are served ----
  int rc = c->finalize_params();
  if (rc != CH_OK) return rc;
  if (c->nwt.path == 2 && c->desc.A.n_unk > 4096) { c->set_err("DC sensitivities: the coupled system has more than 4096 unknowns (dense LU)"); return CH_ERR_UNSUPPORTED; }
  g_arena = &c->arena;
  std::vector<int> status;
  const int rc_dc = c->dc_solve(*o, 0, &status, &st);
  if (rc_dc != CH_OK && status.empty()) return rc_dc;
  const std::string dc_err = c->err();
  const int mode = o->tran_mode ? 2 : 0;
  if (x_out) { rc = c->download_mna(0, 0.0, mode, x_out); if (rc != CH_OK) return rc; }
  const Analysis& A = c->desc.A;
  const int S = c->tab.S, nblk = c->ac_ncomp() * S, ds = c->ac_ds(), nm = A.n_mna;
  if (status_out) for (int s = 0; s < S; ++s) status_out[s] = status[s];
  st.dc_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  c->stats.end_of_dc(st.n_block_iters);
  // ---- G and F at the operating point ----
  const size_t nA = (size_t)nblk * ds * ds, nF = (size_t)nblk * ds;
  auto set_err = [&](const std::string& m) { c->set_err(m); };
  HIPCHK(c->ac.d_dumpG.alloc(nA)); HIPCHK(c->ac.d_dumpC.alloc(nA)); HIPCHK(c->ac.d_dumpA.alloc(nA)); HIPCHK(c->ac.d_dumpF0.alloc(nF)); HIPCHK(c->ac.d_dumpQ.alloc(nF));
  HIPCHK(c->sens.d_Fp.alloc(nF * n_par)); HIPCHK(c->sens.d_Fm.alloc(nF * n_par)); HIPCHK(c->sens.d_x.alloc((size_t)S * n_par * A.n_unk));
  rc = sens_eval(c, c->nwt.base, c->own_sources(), 0, mode, c->ac.d_dumpF0.p, true);
  if (rc != CH_OK) return rc;
  // ---- right-hand sides: residual-only differences ----
  const auto t1 = hclock::now();
  std::vector<double> den((size_t)n_par * S), dsrc((size_t)n_par * S, 0.0), val(S);
  std::vector<int> src_of(n_par, -1);
  const std::vector<char> src_nl = sens_sources_feeding_nonlinear(A, (int)c->desc.src.size());
  int n_eval = 0;
  for (int k = 0; k < n_par; ++k) {
    const int id = slot_ids[k], kind = c->desc.slot_kind[id], sa = c->desc.slot_a[id];
    const int dkind = kind == CH_SLOT_DEV_PAR ? c->desc.dev[sa].kind : 0;
    std::vector<SensStep> step(S);
    const bool snl = (kind == CH_SLOT_SRC_DC || kind == CH_SLOT_SRC_PAR) && src_nl[sa];
    for (int s = 0; s < S; ++s) step[s] = sens_step(kind, dkind, A.wide, snl, c->slot_value(id, s), sopt.rel_step, sopt.abs_step ? sopt.abs_step[k] : 0.0);
    const bool central = step[0].central;   // the kind of difference is a property of the slot, not of the sample
    for (int s = 0; s < S; ++s) den[(size_t)k * S + s] = central ? 2.0 * step[s].h : step[s].h;
    for (int sign = +1; sign >= (central ? -1 : +1); sign -= 2) {
      for (int s = 0; s < S; ++s) val[s] = c->slot_value(id, s) + sign * step[s].h;
      NewtonArgs a = c->nwt.base;
      TableOverride o;
      rc = sens_perturb(c, id, val, o, a);
      if (rc != CH_OK) return rc;
      const SourceTables own = c->own_sources(), src{o.src_dc.empty() ? own.dc : &o.src_dc, o.src_par.empty() ? own.par : &o.src_par};
      rc = sens_eval(c, a, src, o.lds_extra_doubles * sizeof(double), mode, (sign > 0 ? c->sens.d_Fp.p : c->sens.d_Fm.p) + (size_t)k * nF, false);
      if (rc != CH_OK) return rc;
      if (sign > 0 && (kind == CH_SLOT_SRC_DC || kind == CH_SLOT_SRC_PAR)) {
        // d(source value)/dp for the rows of known nodes: 1 where the slot IS the value, otherwise the same forward difference
        src_of[k] = sa;
        const int nsrc = (int)c->desc.src.size();
        for (int s = 0; s < S; ++s) {
          const size_t at = (size_t)(c->tab.Ssrc > 1 ? s : 0) * nsrc + sa;
          const bool is_value = kind == CH_SLOT_SRC_DC && (mode == 0 || c->desc.src[sa].kind == CH_SRC_DC);
          if (is_value) { dsrc[(size_t)k * S + s] = 1.0; continue; }
          const double vp = source_value(c->desc.src[sa], &(*src.par)[at * CH_SRC_NPAR], (*src.dc)[at], 0.0, mode);
          const double v0 = source_value(c->desc.src[sa], &(*own.par)[at * CH_SRC_NPAR], (*own.dc)[at], 0.0, mode);
          dsrc[(size_t)k * S + s] = (vp - v0) / step[s].h;
        }
      }
      ++n_eval;
    }
    if (!central) HIPCHK(hipMemcpyAsync(c->sens.d_Fm.p + (size_t)k * nF, c->ac.d_dumpF0.p, nF * sizeof(double), hipMemcpyDeviceToDevice, c->ctx->stream));
  }
  const auto t2 = hclock::now();
  // ---- the solves ----
  std::vector<int> skip(S, 0), zero(1, 0);
  for (int s = 0; s < S; ++s) skip[s] = status[s] != CH_OK;
  HIPCHK(c->sens.d_den.upload(den, c->ctx->stream)); HIPCHK(c->sens.d_skip.upload(skip, c->ctx->stream)); HIPCHK(c->sens.d_fail.upload(zero, c->ctx->stream));
  SensArgs a; std::memset(&a, 0, sizeof(a));
  a.bmeta = c->ac_bmeta(); a.G = c->ac.d_dumpG.p; a.Fp = c->sens.d_Fp.p; a.Fm = c->sens.d_Fm.p; a.den = c->sens.d_den.p; a.skip = c->sens.d_skip.p;
  if (!a.bmeta) return CH_ERR_DEVICE;
  a.f_stride = (long)nF; a.ds = ds; a.S = S; a.n_unk = A.n_unk; a.n_par = n_par; a.x_out = c->sens.d_x.p; a.fail = c->sens.d_fail.p;
  float solve_ms = 0.0f; int n_chunks = 0, n_solve_launches = 0;
  rc = launch_sens(c, a, nblk, n_par, nF, &solve_ms, &n_chunks, &n_solve_launches);
  if (rc != CH_OK) return rc;
  std::vector<double> xs((size_t)S * n_par * A.n_unk);
  int fail = 0;
  if (hipMemcpy(xs.data(), c->sens.d_x.p, xs.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&fail, c->sens.d_fail.p, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { c->set_err("DC sensitivities: reading the result back failed"); return CH_ERR_DEVICE; }
  // ---- unknown order -> MNA order ----
  for (int s = 0; s < S; ++s) for (int k = 0; k < n_par; ++k)
    sens_expand_mna(A, skip[s] ? nullptr : &xs[((size_t)s * n_par + k) * A.n_unk], src_of[k], dsrc[(size_t)k * S + s], sens_out + ((size_t)s * n_par + k) * nm);
  st.wall_seconds = std::chrono::duration<double>(hclock::now() - t0).count();
  c->stats.fill(st);   // step_kernel_*: the evaluation launches behind the operating point
  st.device_seconds += solve_ms * 1e-3;
  st.n_kernel_launches = c->stats.n_launch + n_solve_launches; st.nf += (int64_t)(n_eval + 1) * S; st.njacs += S; st.nfactors += (int64_t)nblk * n_chunks;
  st.nsolve += (int64_t)nblk * n_par;
  if (c->host_profile)
    std::fprintf(stderr, "[sens] operating point %.3f ms, %d evaluation launches %.3f ms (host wall), solve kernel %.3f ms (HIP events), total %.3f ms\n", st.dc_seconds * 1e3, n_eval,
                 std::chrono::duration<double>(t2 - t1).count() * 1e3, (double)solve_ms, st.wall_seconds * 1e3);
  if (stats) *stats = st;
  if (fail) { c->set_err("DC sensitivities: singular Jacobian G at the operating point"); return CH_ERR_SINGULAR; }
  if (rc_dc != CH_OK) c->set_err(dc_err);
  return rc_dc;
}
}  // extern "C++"
