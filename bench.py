#!/usr/bin/env python3
"""bench.py — Newton iterations/sec and wall-clock per transient on the GF180 DFF array.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N > 1 launched through
`python -m torch.distributed.run --nproc-per-node N …`, one rank per GPU.

Workload (BASELINE.json metric / SURVEY §8(d) config 3): tiled array of 1024 GF180 D-flip-flops
(30 720 BSIM4 MOSFETs, 11 264 unknowns after structural reduction = 1024 independent 11x11 Jacobian
blocks), full transient 0..700 ns with the reference test bench's CLKN/D stimuli,
abstol = reltol = 1e-4 (benchmarks/gf180_dff_solver_bench.jl:27,62), DC operating point included.
A "step" is ONE such transient.  With N GPUs every rank integrates its own process-variation sample
of the array (weak scaling, no data-path collective; the per-rank Q waveforms at the reference's
check times and the iteration counts are gathered once at the end over RCCL).

value = Newton iterations (of the whole array, i.e. max over blocks per step attempt, summed over
ranks) / wall seconds, with the circuit description already resident on the GPU.

`--gpus N` means N: started WITHOUT a launcher (no WORLD_SIZE in the environment) and N > 1, this process starts the N ranks
itself as a child (`python -m torch.distributed.run --nproc-per-node N bench.py ...`) before anything touches the GPU, relays
rank 0's JSON line and exits with the child's code; started under a launcher whose WORLD_SIZE differs from --gpus it refuses.

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds the separate measurements: the measured
triad / fp64 peaks of the roofline, the skewed-clock and coupled-rails variants and the CPU baseline (one GPU), and with N > 1
`config4_sharded_sweep`: the 8192-sample-class Monte-Carlo sweep of SURVEY 8(d) config 4 at 1024 samples per rank through
`CircuitSweep(rank, world)`, with the full result rows [samples x observables x save points] gathered by ONE all_gather over
RCCL (last row).

`--dump-outputs DIR` writes, after the timed steps, what rank 0's last timed transient returned to its caller: the time points
(`t.npy`), the observed Q waveform of tile 0 (`q0.npy`) and the final state vector without the branch currents the engine
eliminated, which it reports as NaN (`final_state.npy`), all float64.  The inputs are deterministic, so two builds can be compared
output for output.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

N_TILES = 1024
TOL = 1e-4
MOS_PER_TILE = 30


def algorithmic_bytes_per_block_iteration(nc, n_mos):
    """eval 400 B/instance (T=4), assembly 288 B/instance + 8(nnz(A)+n),
    LU refactor 8(nnz(A)+2 nnz(L+U)) + solve 8(2 nnz(L+U)+4n); dense block: nnz = nc^2."""
    nnz = nc * nc
    return n_mos * 400 + n_mos * 288 + 8 * (nnz + nc) + 8 * (nnz + 2 * nnz) + 8 * (2 * nnz + 4 * nc)


def _oracle_worker(args):
    """One host thread: full transients of one decoupled DFF tile until the deadline (ctypes releases the GIL)."""
    deadline, max_reps = args[0], args[1]
    proxy = len(args) > 2 and args[2]
    from oracle_binding import Oracle
    from cedarsim_jl_amd import dc_opts, tran_opts
    from cedarsim_jl_amd.workloads import DFF_TSPAN, dff_array
    o = Oracle(dff_array(1))
    o.set_proxy(proxy)
    iters = reps = 0
    while True:
        rc, t, v, xf, st = o.tran(DFF_TSPAN[0], DFF_TSPAN[1], tran_opts(abstol=TOL, reltol=TOL, dc=dc_opts(abstol=1e-14)))
        assert rc == 0
        iters += st["nnonliniter"]
        reps += 1
        if time.perf_counter() > deadline or reps >= max_reps:
            break
    return iters, reps


def cpu_baseline(seconds_single=5.0, seconds_multi=10.0, seconds_proxy=5.0):
    """Oracle ("port") timed on the host cores on a bounded sample: full transients of single decoupled tiles
    (1 of the 1024), first on one core, then one tile per thread on every core this process may use;
    converted to array-level iterations/s by dividing the tile rate by the tile count."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    t0 = time.perf_counter()
    it1, reps1 = _oracle_worker((t0 + seconds_single, 200))
    el1 = time.perf_counter() - t0
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1
    cores = max(1, min(cores, 64))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        res = list(ex.map(_oracle_worker, [(t0 + seconds_multi, 400)] * cores))
    elm = time.perf_counter() - t0
    itm, repsm = sum(r[0] for r in res), sum(r[1] for r in res)
    tile_rate_1, tile_rate_m = it1 / el1, itm / elm
    # B0: "reference-like" cost proxy on one core — finite-difference Jacobian from n+1 residuals, reused like
    # IDA's modified Newton (src/dcop.jl:28,53-94; benchmarks/gf180_dff_solver_bench.jl:60-81), one tile, scaled by the tile
    # count.  Flattering to the reference: its dense LU is O(n^3) of the WHOLE 13.3k system, here it is 25x25 per tile.
    t0 = time.perf_counter()
    itp, repsp = _oracle_worker((t0 + seconds_proxy, 200, True))
    elp = time.perf_counter() - t0
    # the term the per-tile proxy leaves out: IDA's dense LU is of the WHOLE system (`solve(prob, IDA())` uses Sundials' dense
    # default).  One LAPACK dgetrf of a random 4096 x 4096 matrix is timed on this host (a few seconds) and scaled by (13 312 / 4096)^3
    # to the size of the array's system — an extrapolation, labelled as one; the full size is 1.6 TFLOP per refactorisation
    dense_lu = None
    try:
        import numpy as _np
        import scipy.linalg as _sl
        n_meas, n_full = 4096, 13 * N_TILES
        _m = _np.random.default_rng(0).standard_normal((n_meas, n_meas))
        _t0 = time.perf_counter()
        _sl.lu_factor(_m, overwrite_a=True, check_finite=False)
        _el = time.perf_counter() - _t0
        dense_lu = {"n_measured": n_meas, "seconds_measured": _el, "n_full": n_full, "seconds_full_extrapolated_cubic": _el * (n_full / n_meas) ** 3,
                    "what": "scipy.linalg.lu_factor (LAPACK dgetrf as this numpy/scipy build runs it on the host's cores): what ONE Jacobian refresh of "
                            "IDA's dense default adds per refactorisation of the whole array; not included in `value`"}
        del _m
    except Exception as ex:  # noqa: BLE001
        dense_lu = {"error": "%s: %s" % (type(ex).__name__, ex)}
    proxy = {"kind": "proxy, not CedarSim", "value": itp / elp / N_TILES, "dense_lu_of_the_whole_system": dense_lu, "unit": "newton_iters/s (1024-DFF array equivalent)", "cores": 1,
             "seconds_per_tile_transient": elp / repsp, "seconds_per_array_transient_scaled": elp / repsp * N_TILES,
             "sample": "%d full transients of one decoupled tile with a finite-difference Jacobian (26 residuals each) reused across "
                       "iterations and steps, %.1f s" % (repsp, elp)}
    return {"value": tile_rate_m / N_TILES, "reference_like_proxy_B0": proxy, "unit": "newton_iters/s (1024-DFF array equivalent)", "cores": cores, "kind": "port",
            "sample": "%d full transients of single decoupled DFF tiles (1 of the %d; dense-LU MNA oracle, n=25) on %d threads, "
                      "%.1f s; tile rate %.0f iters/s divided by %d" % (repsm, N_TILES, cores, elm, tile_rate_m, N_TILES),
            "single_core_value": tile_rate_1 / N_TILES, "seconds_per_tile_transient_single_core": el1 / reps1}


def combine_ranks(dist, world, device, iters, el, gate_ok, q):
    """The only collective of the bench: one all_gather of a small per-rank vector AFTER the timed region (RCCL over xGMI when
    `device` is a GPU, gloo on the CPU rehearsal).  Returns whole-job iterations (sum over ranks), the slowest rank's time
    (max), the AND of the ranks' gates, and every rank's gate values."""
    import torch
    if dist is None or world <= 1:
        return float(iters), el, bool(gate_ok), [list(q)]
    buf = torch.tensor([float(iters), el, float(gate_ok)] + list(q), dtype=torch.float64, device=device)
    out = [torch.zeros_like(buf) for _ in range(world)]
    dist.all_gather(out, buf)  # result gather only
    res = torch.stack(out).cpu().numpy()
    return float(res[:, 0].sum()), float(res[:, 1].max()), bool(res[:, 2].min() > 0.5), res[:, 3:].tolist()


def launch_ranks(n, argv):
    """Parent of a launcher-less `bench.py --gpus N` (N > 1): no torch.cuda / HIP call has happened in this process.  The ranks
    run in a CHILD process tree (never exec: the GPU box forbids replacing a process that may have touched the GPU)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    relayed = 0
    for ln in proc.stdout:
        if ln.startswith('{"metric"'):
            sys.stdout.write(ln)
            sys.stdout.flush()
            relayed += 1
        else:
            sys.stderr.write(ln)
    rc = proc.wait()
    if rc == 0 and relayed != 1:
        sys.stderr.write("bench.py: expected one JSON line from rank 0, saw %d\n" % relayed)
        rc = 3
    return rc


def config4_sharded_sweep(ctx, rank, world, dist, backend, samples_per_rank=1024, n_save=2001, plumbing_only=False):
    """an explicit Monte-Carlo TandemSweep of one DFF (src/sweeps.jl:278-290, 471-502), 1024 samples per
    rank, sharded by `CircuitSweep(rank, world)` (contiguous blocks of points), every rank's share ONE batched solve on the
    device-resident stepper with per-sample steps, output on a saveat grid; then the collective of the path: ONE all_gather of the
    rows [samples, observables, save points] (RCCL over xGMI with the nccl backend).  Returns the rank-0 report."""
    import numpy as np
    import torch
    from cedarsim_jl_amd import CircuitSweep, gather_sharded
    from cedarsim_jl_amd.workloads import DFF_CHECK_Q, DFF_CHECK_TIMES, DFF_TSPAN, dff_mc_builder, mc_tandem_sweep
    S_total = samples_per_rank * world
    saveat = np.unique(np.concatenate((np.linspace(DFF_TSPAN[0], DFF_TSPAN[1], n_save), np.array(DFF_CHECK_TIMES))))
    build, names = dff_mc_builder(observe=("q", "q_neg"))
    cs = CircuitSweep(build, mc_tandem_sweep(S_total), rank=rank, world=world)
    t0 = time.perf_counter()
    if plumbing_only:   # CPU rehearsal of launcher + gather: rows are a pattern that encodes (sample, observable, save point)
        from cedarsim_jl_amd.sweeps import shard_range
        lo, hi = shard_range(S_total, rank, world)
        rows = (np.arange(lo, hi)[:, None, None] * 1e3 + np.arange(2)[None, :, None] * 1e2 + np.arange(len(saveat))[None, None, :] * 1e-3)
        stats, setup, rc = {"nnonliniter": 0, "dc_seconds": 0.0, "stepper": 0, "stepper_mode": 0}, {"circuit_builds": 0, "seconds": 0.0, "how": "plumbing only"}, 0
    else:
        rc, t, rows, stats = cs.tran_arrays(DFF_TSPAN, abstol=TOL, reltol=TOL, dc_abstol=1e-14, saveat=saveat, ctx=ctx)
        setup = cs.setup
    solve_s = time.perf_counter() - t0
    dev = "cuda" if backend == "nccl" else "cpu"
    if dist is not None:
        dist.barrier()
    if dev == "cuda":
        torch.cuda.synchronize()
    # The gather.  With RCCL the rows go GPU to GPU straight from the engine's result buffer in HBM (ch_result_device_values through
    # `__cuda_array_interface__`: no host round trip); the gathered tensor is copied to the host once afterwards, for the checks below,
    # and that copy is timed apart.  Anything else (the gloo rehearsal, rows the engine did not keep on the device): host rows.
    how, d2h_s = "host rows -> device staging -> all_gather -> host", None
    drows = None if plumbing_only else stats.get("device_rows")
    # The zero-copy view is taken — and the choice of path agreed between the ranks (one tiny all_reduce: a rank that took another
    # path than its peers would hang their collective) — BEFORE the timed gather; a rank that cannot wrap its buffer sends everybody
    # to the host-rows path, and says why.
    local_dev, view_note = None, None
    if dist is not None and dev == "cuda":
        ok_here = 0
        if drows is not None:
            try:
                local_dev = torch.as_tensor(drows, device="cuda")            # zero-copy view of the engine's buffer [n_obs, n_save, samples]
                ok_here = 1 if (tuple(local_dev.shape) == tuple(drows.shape) and local_dev.dtype == torch.float64) else 0
            except Exception as ex:  # noqa: BLE001
                view_note = "%s: %s" % (type(ex).__name__, ex)
        flag = torch.tensor([ok_here], device="cuda", dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0:
            local_dev = None
            how = "host rows -> device staging -> all_gather -> host (no device view of the engine's rows on some rank%s)" % ((": " + view_note) if view_note else "")
    t0 = time.perf_counter()
    if local_dev is not None:
        from cedarsim_jl_amd import gather_sharded_device
        full_dev = gather_sharded_device(local_dev, S_total, rank, world)    # [n_obs, n_save, S_total] on every rank
        torch.cuda.synchronize()
        gather_s = time.perf_counter() - t0
        t1 = time.perf_counter()
        full = np.ascontiguousarray(full_dev.permute(2, 0, 1).cpu().numpy())
        d2h_s = time.perf_counter() - t1
        how = "engine's result buffer in HBM -> all_gather (RCCL, GPU to GPU); device -> host copy of the gathered rows timed apart"
    else:
        full = gather_sharded(rows, S_total, rank, world, device=dev) if dist is not None else rows
        if dev == "cuda":
            torch.cuda.synchronize()
        gather_s = time.perf_counter() - t0
    # every rank holds every sample's rows now: check the reference's gate on ALL of them, and that the shards landed in order
    ci = np.searchsorted(saveat, np.array(DFF_CHECK_TIMES))
    if plumbing_only:
        want = (np.arange(S_total)[:, None, None] * 1e3 + np.arange(2)[None, :, None] * 1e2 + np.arange(len(saveat))[None, None, :] * 1e-3)
        ok = bool(np.array_equal(full, want))
        n_pass = S_total if ok else 0
    else:
        passed = np.all(np.abs(full[:, 0, :][:, ci] - np.array(DFF_CHECK_Q)[None, :]) <= 10 * TOL, axis=1)
        n_pass = int(passed.sum())
        lo = rank * samples_per_rank
        ok = bool(np.array_equal(full[lo:lo + samples_per_rank], rows))
    vec = [solve_s, gather_s, float(rc), float(stats["nnonliniter"]), float(ok), float(setup["seconds"])]
    if dist is not None:
        buf = torch.tensor(vec, dtype=torch.float64, device=dev)
        out = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(out, buf)
        res = torch.stack(out).cpu().numpy()
    else:
        res = np.array([vec])
    bytes_per_rank = int(rows.size * 8)
    return {"workload": "Monte-Carlo TandemSweep of one GF180 DFF (%s), %d samples per rank, %d in total, transient 0..700 ns abstol=reltol=1e-4, "
                        "saveat grid of %d points, %d observables" % (", ".join(names), samples_per_rank, S_total, len(saveat), rows.shape[1]),
            "samples_total": S_total, "samples_per_rank": samples_per_rank, "n_obs": int(rows.shape[1]), "n_save": int(rows.shape[2]),
            "rc_worst": int(res[:, 2].min()), "solve_seconds_max_over_ranks": float(res[:, 0].max()), "sweep_setup_seconds_max_over_ranks": float(res[:, 5].max()),
            "sweep_setup": setup, "newton_iters_total": float(res[:, 3].sum()), "samples_per_second": S_total / float(res[:, 0].max()),
            "gather": {"collective": "one all_gather of [samples/rank, n_obs, n_save] fp64 rows (%s)" % ("RCCL over xGMI" if backend == "nccl" else backend),
                       "bytes_per_rank": bytes_per_rank, "seconds_max_over_ranks": float(res[:, 1].max()),
                       "GBps_per_rank_received": (world - 1) * bytes_per_rank / max(1e-12, float(res[:, 1].max())) / 1e9 if world > 1 else None,
                       "path": how, "device_to_host_seconds_rank0": d2h_s},
            "every_rank_sees_its_shard_in_place": bool(res[:, 4].min() > 0.5), "samples_passing_reference_gate": n_pass,
            "stepper": "device-resident, per-sample step acceptance" if stats.get("stepper") == 2 else ("plumbing only" if plumbing_only else "host"),
            "plumbing_only": bool(plumbing_only)}


def plumbing_only_line(args, rank, world):
    """`--plumbing-only` (hidden; tests/test_capi_and_dist.py): launcher, rendezvous, `combine_ranks` and the full-size config-4
    gather over gloo on a machine without a GPU.  No engine, no oracle, no measurement: `value` is null."""
    import torch.distributed as dist
    d = None
    if world > 1:
        dist.init_process_group(backend="gloo")
        d = dist
    tot, mx, gate, allq = combine_ranks(d, world, "cpu", 1000 + rank, 0.05 + 0.01 * rank, True, [0.0, 0.0, 5.0, 5.0, 5.0])
    c4 = config4_sharded_sweep(None, rank, world, d, "gloo", samples_per_rank=args.mc_samples_per_rank, plumbing_only=True)
    if rank == 0:
        print(json.dumps({"metric": "newton_iters_per_sec", "value": None, "unit": "newton_iters/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "plumbing_only": True, "combined_iters": tot, "slowest_rank_seconds": mx, "config4_sharded_sweep": c4}))
    if d is not None:
        d.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tiles", type=int, default=N_TILES, help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true", help="also run the separate measurements: measured peaks, variants, CPU baseline, config 4")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs (rank 0) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-skew", action="store_true", help="skip the second, clearly labelled measurement with per-tile clock skew")
    ap.add_argument("--stepper", default="auto", choices=["auto", "host", "device"], help=argparse.SUPPRESS)
    ap.add_argument("--mc-samples-per-rank", type=int, default=1024, help=argparse.SUPPRESS)
    ap.add_argument("--plumbing-only", action="store_true", help=argparse.SUPPRESS)   # CPU test of launcher + collectives: no engine, no `value`
    args = ap.parse_args()

    # ---- --gpus N means N ----
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        sys.stderr.write("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks; refusing to report a line for the wrong job size\n"
                         % (args.gpus, os.environ["WORLD_SIZE"]))
        sys.exit(2)

    import numpy as np
    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.plumbing_only:
        return plumbing_only_line(args, rank, world)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device; there is no CPU fallback")
    # CEDARHIP_DIST_BACKEND=gloo is a rehearsal mode for boxes with fewer GPUs than ranks (ranks share devices, the result
    # gather goes through host memory); the driver's multi-GPU runs use the default: one GPU per rank, RCCL over xGMI
    backend = os.environ.get("CEDARHIP_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend=backend)

    from cedarsim_jl_amd import dc_opts, tran_opts
    from cedarsim_jl_amd.engine import Context, EngineCircuit
    from cedarsim_jl_amd.workloads import DFF_CHECK_Q, DFF_CHECK_TIMES, DFF_TSPAN, dff_array

    ctx = Context(local_rank)
    ckt = dff_array(args.tiles, observe="q0")
    # one process-variation sample per rank (seed 2024 + rank): multipliers on vth0/u0 of both cards
    if world > 1:
        rng = np.random.default_rng(2024 + rank)
        slots, vals = [], []
        from cedarsim_jl_amd import bsim4_params as B4
        for mname in ("nfet_06v0", "pfet_06v0"):
            for par in ("vth0", "u0"):
                bv = ckt.models[ckt.model_names.index(mname)][B4.PARAM_INDEX[par]]
                slots.append(ckt.slot(mname, par))
                vals.append([bv * (1.0 + 0.03 * rng.standard_normal())])
    eng = EngineCircuit(ckt, ctx)
    if world > 1:
        eng.set_samples(1)
        eng.set_params(slots, vals)
    info = eng.info()
    opts = tran_opts(abstol=TOL, reltol=TOL, dc=dc_opts(abstol=1e-14), stepper=args.stepper)

    def one_transient(eng=eng):
        rc, t, v, xf, st = eng.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts)
        if rc != 0:
            raise SystemExit("transient failed: rc=%d %s" % (rc, ctx.last_error()))
        q = [float(np.interp(tt, t, v[0, :, 0])) for tt in DFF_CHECK_TIMES]
        return st, q, (t, v, xf)

    for _ in range(args.warmup):
        one_transient()

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    t0 = time.perf_counter()
    iters = block_iters = launches = attempts = 0
    dev_s = dc_s = bar_s = 0.0
    naccept = nreject = 0
    q = out = None
    stepper_used = 0
    for _ in range(args.steps):
        st, q, out = one_transient()
        iters += st["nnonliniter"]
        block_iters += st["step_block_iters"]          # inside the time-stepping kernel(s): what the roofline line is about
        launches += st["step_kernel_launches"]
        dev_s += st["step_kernel_seconds"]
        dc_s += st["dc_seconds"]
        bar_s += st["barrier_seconds"]
        attempts += st["n_step_attempts"]
        naccept += st["naccept"]
        nreject += st["nreject"]
        stepper_used = st["stepper"]
    barrier()
    el = time.perf_counter() - t0

    if args.dump_outputs and rank == 0 and out is not None:
        t, v, xf = out
        # the MNA state holds NaN for branch currents the engine eliminated (no unknown): keep node voltages and solved branches,
        # chosen by the circuit's structure, not by value
        _, _, branch_unknown = eng.maps()
        solved = np.concatenate((np.ones(ckt.n_nodes, bool), branch_unknown >= 0))
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in (("t", t), ("q0", v[0, :, 0]), ("final_state", xf[0][solved])):
            np.save(os.path.join(args.dump_outputs, name + ".npy"), np.ascontiguousarray(arr, dtype=np.float64))

    # correctness gate of the reference harness (benchmarks/gf180_dff_solver_bench.jl:84-96)
    gate_ok = all(abs(a - b) <= 10 * TOL for a, b in zip(q, DFF_CHECK_Q))

    tot_iters, max_el, gate_ok, all_q = combine_ranks(dist, world, "cuda" if backend == "nccl" else "cpu", iters, el, gate_ok, q)

    c4 = None
    if world > 1 and args.full:
        # second, separate measurement (never `value`): the sharded Monte-Carlo sweep with its full-size result gather
        try:
            c4 = config4_sharded_sweep(ctx, rank, world, dist, backend, samples_per_rank=args.mc_samples_per_rank)
        except Exception as ex:  # noqa: BLE001
            if dist is not None and world > 1:
                raise   # a rank that drops out of a collective would hang the others: fail the job loudly instead
            c4 = {"error": "%s: %s" % (type(ex).__name__, ex)}

    if rank == 0:
        nc, n_mos = info["max_component"], MOS_PER_TILE
        bpi = algorithmic_bytes_per_block_iteration(nc, n_mos)
        avg_launch = dev_s / max(1, launches)
        bytes_per_launch = bpi * block_iters / max(1, launches)
        achieved = bytes_per_launch / avg_launch / 1e9 if avg_launch > 0 else 0.0
        # HBM traffic and the fp64 instruction mix come from separate rocprofv3 --pmc passes (scripts/profile_round.sh); they
        # are quoted only when that file was measured on THIS build of the library (hash of the .so) and this stepper
        traffic = flops = None
        pmc_note = "no PMC file for this build"
        import hashlib
        from cedarsim_jl_amd import engine as _eng
        lib_hash = hashlib.sha256(open(_eng.LIB_PATH, "rb").read()).hexdigest()
        for cand in sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith("_pmc_traffic.json")):
            try:
                pj = json.load(open(os.path.join(ROOT, "profiles", cand)))
            except Exception:  # noqa: BLE001
                continue
            if pj.get("lib_sha256") == lib_hash and pj.get("tiles", N_TILES) == args.tiles and "bench.py" in pj.get("workload", "bench.py") \
                    and pj.get("kernel", "") in ("tran_persistent_kernel", "newton_block_kernel"):
                traffic = pj.get("hbm_bytes_per_launch")
                flops = pj.get("fp64_flop_per_launch")
                pmc_note = "profiles/%s (same library build, sha256 %s...)" % (cand, lib_hash[:12])
        triad = fp64_peak = None
        if args.full:   # microbenchmarks of their own
            try:
                triad, fp64_peak = ctx.triad_gbps(), ctx.fp64_tflops()
            except RuntimeError:
                pass
        line = {
            "metric": "newton_iters_per_sec", "value": tot_iters / max_el, "unit": "newton_iters/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * max_el / max(1, args.steps),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "gf180_dff_array_%d tiles transient 0..700ns abstol=reltol=1e-4 (SURVEY 8d config 3)" % args.tiles,
                       "tiles": args.tiles, "mosfets": args.tiles * MOS_PER_TILE, "unknowns": info["n_unknowns"],
                       "blocks": info["n_components"], "block_size": nc, "device_cards": "substitute BSIM4 cards (GF180MCUPDK unavailable)",
                       "wall_seconds_per_transient": max_el / max(1, args.steps),
                       "dc_seconds_per_transient": dc_s / max(1, args.steps),
                       "tile_newton_iters_per_sec": tot_iters * args.tiles / max_el,
                       "accepted_steps": naccept // max(1, args.steps), "rejected_steps": nreject // max(1, args.steps),
                       "reference_gate_q": all_q[0], "reference_gate_ok": gate_ok,
                       "step_controller": "device-resident (one persistent cooperative launch per transient)" if stepper_used == 2 else "host (one launch per attempt)",
                       "multi_gpu": "independent process-variation samples per rank; all_gather of results only"},
            "roofline": {"bound": "hbm", "kernel": "tran_persistent_kernel (one launch per transient)" if stepper_used == 2 else "newton_block_kernel (one launch per step attempt)",
                         "achieved": achieved, "peak": 8000.0, "unit": "GB/s",
                         "frac": achieved / 8000.0, "traffic": traffic, "traffic_source": pmc_note,
                         "measured_hbm_gbps": (traffic / avg_launch / 1e9) if (traffic and avg_launch > 0) else None,
                         "limiter": "fp64 VALU issue + dependency latency (one wave per SIMD); HBM is the stated bound of the path, not the limiter here",
                         # what the two headline fields are, by name: `achieved`/`frac` = ALGORITHMIC bytes (SURVEY 8(d) formula) over kernel time
                         # against 8 TB/s — the contract's figure, not a measured HBM rate (that is `measured_hbm_gbps`); the honest
                         # utilisation figure of this fp64-issue-bound kernel is `frac_fp64_issue`
                         "algorithmic_gbps": achieved,
                         "frac_fp64_issue": ((flops / avg_launch / 1e12) / fp64_peak) if (flops and avg_launch > 0 and fp64_peak) else None,
                         "step_attempts_per_launch": attempts / max(1, launches), "us_per_step_attempt": 1e6 * dev_s / max(1, attempts),
                         "grid_reduction_us_per_attempt": 1e6 * bar_s / max(1, attempts),
                         "algorithmic_bytes_per_block_iteration": bpi, "block_iterations_per_launch": block_iters / max(1, launches),
                         "avg_launch_us": 1e6 * avg_launch, "launches": launches,
                         "peak_measured_triad": triad, "frac_of_measured_triad": (achieved / triad) if triad else None,
                         "fp64_tflops_achieved": (flops / avg_launch / 1e12) if (flops and avg_launch > 0) else None,
                         "fp64_vector_peak_tflops_measured": fp64_peak,
                         "note": "stamps and the block Jacobian stay in LDS, so HBM is not the limiter; the kernel is "
                                 "fp64-VALU/latency bound (see DESIGN.md)"},
        }
        # The two variants below are separate, clearly labelled measurements; a failure inside one of them is reported in its field
        # and never costs the headline line.
        if args.full and world == 1 and not args.no_skew and args.tiles == N_TILES:
            try:
                # SURVEY 8(d) config 3 variant: per-tile clock skew U(0, 50 ps), seed 1234 — every tile has its own clock source, the
                # tiles stop being bit-identical (the worst case for one shared step size).  A second, separate measurement: NOT `value`.
                rngs = np.random.default_rng(1234)
                ck = dff_array(args.tiles, skew=rngs.uniform(0.0, 50e-12, args.tiles), observe="q")
                es = EngineCircuit(ck, ctx)
                # output on a saveat grid (the gate times): independent blocks then take their own steps — no tile pays for the
                # other 1023 clocks' corners (lock-step, every accepted step saved: 62 292 steps, 4.3 s; profiles/r02_notes.md)
                opts_s = tran_opts(abstol=TOL, reltol=TOL, dc=dc_opts(abstol=1e-14), stepper=args.stepper, saveat=np.array(DFF_CHECK_TIMES))
                es.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts_s)
                t0s = time.perf_counter()
                rc_s, t_s, v_s, _, st_s = es.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts_s)
                el_s = time.perf_counter() - t0s
                qs = np.array([[np.interp(tt, t_s, v_s[k, :, 0]) for tt in DFF_CHECK_TIMES] for k in range(v_s.shape[0])])
                # for comparison, ONE run with every accepted step of ONE step sequence saved (what a caller without saveat gets):
                # 1024 private clocks are more than the device-resident controller's 64 lock-step sources, so this is the host stepper
                t0l = time.perf_counter()
                rc_l, t_l, v_l, _, st_l = es.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts)
                el_l = time.perf_counter() - t0l
                line["skewed_clock_variant"] = {"workload": "same array, per-tile clock skew U(0,50 ps) seed 1234 (%d private clock sources)" % args.tiles,
                                                "rc": rc_s, "ms_per_transient": 1e3 * el_s, "newton_iters_per_sec_slowest_block": st_s["nnonliniter"] / el_s,
                                                "note": "own steps: nnonliniter is the slowest block's count — not comparable with the headline's array-level iterations/s",
                                                "accepted_steps": st_s["naccept"], "rejected_steps": st_s["nreject"], "step_attempts": st_s["n_step_attempts"],
                                                "step_controller": "device-resident, per-block step acceptance on the saveat grid of the gate times" if st_s["stepper"] == 2 else "host, lock-step",
                                                "block_iterations": st_s["n_block_iters"],
                                                "lockstep_every_step_saved": {"rc": rc_l, "ms_per_transient": 1e3 * el_l, "accepted_steps": st_l["naccept"], "rejected_steps": st_l["nreject"],
                                                                              "block_iterations": st_l["n_block_iters"], "step_controller": "device-resident" if st_l["stepper"] == 2 else "host"},
                                                "every_tile_meets_reference_gate": bool(np.max(np.abs(qs - np.array(DFF_CHECK_Q)[None, :])) <= 10 * TOL)}
            except Exception as ex:  # noqa: BLE001
                line["skewed_clock_variant"] = {"error": "%s: %s" % (type(ex).__name__, ex)}
        if args.full and world == 1 and not args.no_skew and args.tiles == N_TILES:
            try:
                # The same array behind NON-IDEAL rails (1 ohm in series with VDD and VSS): structurally ONE coupled block of 11 266
                # unknowns — "assembly + LU refactor" of BASELINE.json config 3 taken literally.  The engine tears it at the two rail
                # unknowns: register LU per tile + Schur complement on the rails inside the device-resident stepper, DC on the sparse
                # path.  A third, separate measurement: NOT `value`.
                cc = dff_array(args.tiles, observe="q", supply_r=1.0)
                ec = EngineCircuit(cc, ctx)
                # DC tolerance 1e-12 A: a rail row sums the currents of 15 360 MOSFET terminals, its residual has a rounding floor near 1e-13
                # (output on the gate times: with every accepted step of 1024 observables saved, 9 MB of rows per transient cross PCIe)
                opts_c = tran_opts(abstol=TOL, reltol=TOL, dc=dc_opts(abstol=1e-12), stepper=args.stepper, saveat=np.array(DFF_CHECK_TIMES))
                ec.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts_c)
                t0c = time.perf_counter()
                rc_c, t_c, v_c, _, st_c = ec.tran(DFF_TSPAN[0], DFF_TSPAN[1], opts_c)
                el_c = time.perf_counter() - t0c
                qc = np.array([[np.interp(tt, t_c, v_c[k, :, 0]) for tt in DFF_CHECK_TIMES] for k in range(v_c.shape[0])])
                ic = ec.info()
                line["coupled_rails_variant"] = {"workload": "same array, 1 ohm in series with the VDD and VSS sources (one coupled block, %d unknowns, nnz(J) %d)" % (ic["n_unknowns"], ic["nnz_jac"]),
                                                 "rc": rc_c, "ms_per_transient": 1e3 * el_c, "dc_ms": 1e3 * st_c["dc_seconds"], "newton_iters_per_sec": st_c["nnonliniter"] / el_c,
                                                 "accepted_steps": st_c["naccept"], "rejected_steps": st_c["nreject"], "step_attempts": st_c["n_step_attempts"],
                                                 "solver": "torn at the rails: register LU per tile + Schur complement, device-resident stepper" if st_c["stepper"] == 2 else "sparse path (level-synchronous LU), host stepper",
                                                 "every_tile_meets_reference_gate": bool(np.max(np.abs(qc - np.array(DFF_CHECK_Q)[None, :])) <= 10 * TOL)}
            except Exception as ex:  # noqa: BLE001
                line["coupled_rails_variant"] = {"error": "%s: %s" % (type(ex).__name__, ex)}
        if c4 is not None:
            line["config4_sharded_sweep"] = c4
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                line["cpu_baseline"] = cpu_baseline()
            except Exception as ex:  # noqa: BLE001  (the oracle library is test infrastructure: its absence must not cost the GPU line)
                line["cpu_baseline"] = {"value": None, "unit": "newton_iters/s", "cores": 0, "kind": "port", "sample": "not measured", "error": "%s: %s" % (type(ex).__name__, ex)}
        else:
            line["cpu_baseline"] = None
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
