/* cedarhip.h — C-ABI of the MI355X-native transient/DC Newton engine for CedarSim-style circuits.
 *
 * This is the drop-in boundary described in DESIGN.md §2.  CedarSim (Julia) has NO FFI for this
 * path today (the only ccall in the reference is :jl_generating_output, src/CedarSim.jl:44); the
 * hot path runs inside un-vendored Julia/C packages (DAECompiler, Sundials IDA, NonlinearSolve).
 * Each entry point below therefore cites the reference *interface* whose work it replaces; the
 * Julia-side binding a maintainer would add is shown in INTEGRATION.md and cedarsim.jl_amd/julia/.
 *
 * Conventions
 *   - plain C, no torch types; all arrays are caller-owned and copied by the engine unless stated.
 *   - node ids: 0 is ground, 1..n_nodes are circuit nodes.
 *   - MNA solution vectors ("x_mna") have length n_nodes + n_branches:
 *       x_mna[0..n_nodes)            node voltages of node 1..n_nodes
 *       x_mna[n_nodes + k]           current of the k-th branch device (V, L, E in device order),
 *                                    flowing from net+ to net- through the device — the sign
 *                                    convention of branch!() (src/simulate_ir.jl:112-120).
 *   - all functions return 0 on success or a negative CH_ERR_* code; they never throw: every entry point catches
 *     C++ exceptions at the boundary (CH_ERR_NOMEM / CH_ERR_INTERNAL; builders return NULL), the way CedarDCOp
 *     swallows solver exceptions and reports a retcode (src/dcop.jl:58-82).
 *   - a ch_ctx / ch_circuit is not thread-safe; use one host thread per GPU (one process per GPU).
 */
#ifndef CEDARHIP_H
#define CEDARHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CH_NAN (__builtin_nan(""))

/* ---- error codes (map to SciML retcodes on the Julia side) ---- */
enum {
  CH_OK = 0,
  CH_ERR_INVALID = -1,      /* bad argument / malformed description (CedarError)            */
  CH_ERR_SINGULAR = -2,     /* singular Jacobian (LinearAlgebra.SingularException)          */
  CH_ERR_MAXITERS = -3,     /* DC did not converge: ReturnCode.InitialFailure / MaxIters    */
  CH_ERR_DTMIN = -4,        /* step size underflow: ReturnCode.DtLessThanMin                */
  CH_ERR_DEVICE = -5,       /* HIP runtime failure                                          */
  CH_ERR_UNSUPPORTED = -6,  /* feature outside the engine's scope                           */
  CH_ERR_MAXSTEPS = -7,     /* transient exceeded max_steps: ReturnCode.MaxIters            */
  CH_ERR_NOMEM = -8,        /* host allocation failed inside the call (std::bad_alloc / length_error) */
  CH_ERR_INTERNAL = -9      /* any other C++ exception caught at the boundary (message in ch_last_error) */
};

/* ---- device kinds (reference device functors, src/simpledevices.jl, src/vasim.jl) ---- */
enum {
  CH_DEV_R = 1,    /* SimpleResistor   simpledevices.jl:65-77   par[0]=r                      */
  CH_DEV_C = 2,    /* SimpleCapacitor  simpledevices.jl:105-109 par[0]=c                      */
  CH_DEV_L = 3,    /* SimpleInductor   simpledevices.jl:128-132 par[0]=l     (branch)         */
  CH_DEV_V = 4,    /* VoltageSource    simpledevices.jl:288-300 ipar[0]=source (branch)       */
  CH_DEV_I = 5,    /* CurrentSource    simpledevices.jl:327-339 ipar[0]=source                */
  CH_DEV_VCVS = 6, /* vcvs             simpledevices.jl:347-356 par[0]=gain  (branch)         */
  CH_DEV_VCCS = 7, /* vccs             simpledevices.jl:364-373 par[0]=gain                   */
  CH_DEV_MOS = 8,  /* BSIM4 functor (VA-generated in the reference, vasim.jl:853-867):
                      nodes d,g,s,b ; ipar[0]=model ; par = {w,l,nf,as,ad,ps,pd,-}            */
  CH_DEV_VA = 9    /* compiled Verilog-A module (device functor of make_spice_device, vasim.jl:649-867):
                      nodes = ports then internal nets (the caller allocates the internal nets as
                      circuit nodes) ; ipar[0] = module id (ch_va_find) ; ipar[1] = offset of the
                      instance's parameter block in ch_desc.va_par                              */
};
#define CH_DEV_NNODE 8
#define CH_DEV_NPAR 8
#define CH_DEV_NIPAR 2

/* MOS instance parameter slots inside par[] */
enum { CH_MOS_W = 0, CH_MOS_L = 1, CH_MOS_NF = 2, CH_MOS_AS = 3, CH_MOS_AD = 4, CH_MOS_PS = 5, CH_MOS_PD = 6 };

/* ---- source waveforms (src/spectre_env.jl:144-176) ---- */
enum {
  CH_SRC_DC = 0,
  CH_SRC_PWL = 1,   /* pwl(wave)            spectre_env.jl:43-69,144-151 */
  CH_SRC_PULSE = 2, /* pulse(v1,v2,td,tr,tf,pw,period)  :153-166 ; par = v1 v2 td tr tf pw period */
  CH_SRC_SIN = 3    /* spsin(vo,va,freq,td,theta,phase,ncycles) :169-176                           */
};
#define CH_SRC_NPAR 8

/* ---- BSIM4 model-card parameter indices ---- */
enum {
#define P(n, d) CH_B4_##n,
#define B(n, d) CH_B4_##n, CH_B4_l##n, CH_B4_w##n, CH_B4_p##n,
#define I(n)
#include "cedarhip_bsim4_params.def"
  CH_B4_NPAR
};

/* ---- BSIM4 noise parameters: not part of ch_desc.model_par (the .def lists them as accepted and ignored there); they reach the
 * noise analysis through ch_set_mos_noise, one row of CH_B4N_NPAR doubles per model card, NaN = not given ---- */
enum {
  CH_B4N_noia, CH_B4N_noib, CH_B4N_noic, CH_B4N_em, CH_B4N_ef, CH_B4N_af, CH_B4N_kf, CH_B4N_ntnoi, CH_B4N_tnoia, CH_B4N_tnoib,
  CH_B4N_rnoia, CH_B4N_rnoib, CH_B4N_fnoimod, CH_B4N_tnoimod, CH_B4N_NPAR
};
/* operand row of one MOSFET noise evaluation (ch_noise_sources, mos_operands): mode-frame quantities at the operating point */
#define CH_B4N_NOPERAND 16

/* ---- sweepable parameter slots: the runtime fields of ParamSim's `p` (circuitodesystem.jl:66-97) ---- */
enum {
  CH_SLOT_DEV_PAR = 1,   /* a = device index, b = par index            */
  CH_SLOT_MODEL_PAR = 2, /* a = model index,  b = CH_B4_* index        */
  CH_SLOT_SRC_DC = 3,    /* a = source index  (dc AND constant tran)   */
  CH_SLOT_SRC_PAR = 4,   /* a = source index, b = par index            */
  CH_SLOT_TEMP = 5,      /* SimSpec.temp  (simulate_ir.jl:15)          */
  CH_SLOT_GMIN = 6,      /* SimSpec.gmin  (simulate_ir.jl:16)          */
  CH_SLOT_DEV_MULT = 7,  /* a = device index: ParallelInstances m      */
  CH_SLOT_VA_PAR = 8     /* a = index into ch_desc.va_par (one entry of a compiled Verilog-A instance's parameter block) */
};

/* Flat circuit description = what a StampExtract overlay over the netlist closure records
 * (SURVEY §3.5): device type, field values, net ids, multiplier. */
typedef struct ch_desc {
  int32_t n_nodes; /* excluding ground */
  /* devices */
  int32_t n_dev;
  const int32_t* dev_kind; /* [n_dev] CH_DEV_*                                   */
  const int32_t* dev_node; /* [n_dev*CH_DEV_NNODE] node ids (unused = 0)         */
  const int32_t* dev_ipar; /* [n_dev*CH_DEV_NIPAR]                               */
  const double* dev_par;   /* [n_dev*CH_DEV_NPAR] (NaN = not given)              */
  const double* dev_mult;  /* [n_dev] multiplicity m (simulate_ir.jl:56-75)      */
  /* sources */
  int32_t n_src;
  const int32_t* src_kind;    /* [n_src] CH_SRC_* : transient waveform            */
  const double* src_dc;       /* [n_src] value in :dcop mode (simpledevices.jl:290-291) */
  const double* src_par;      /* [n_src*CH_SRC_NPAR]                              */
  const int32_t* src_pwl_ofs; /* [n_src+1] offsets into pwl_t/pwl_y               */
  const double* pwl_t;
  const double* pwl_y;
  /* BSIM4 model cards */
  int32_t n_model;
  const double* model_par; /* [n_model*CH_B4_NPAR], NaN = not given */
  /* SimSpec (simulate_ir.jl:12-20) */
  double temp;  /* Celsius, default 27 */
  double gmin;  /* default 1e-12       */
  double scale; /* default 1           */
  /* sweepable slots */
  int32_t n_slot;
  const int32_t* slot_kind; /* [n_slot] CH_SLOT_* */
  const int32_t* slot_a;    /* [n_slot] */
  const int32_t* slot_b;    /* [n_slot] */
  /* observables saved by ch_tran: node voltages and branch currents */
  int32_t n_obs;
  const int32_t* obs_kind;  /* [n_obs] 0 = node voltage (index = node id), 1 = branch current (index = device index) */
  const int32_t* obs_index; /* [n_obs] */
  /* small-signal analysis: |ac| of every source (VoltageSource/CurrentSource `ac`, the phase is ignored as
   * in src/simpledevices.jl:293,332), or NULL when no source has one.  A voltage source with ac != 0 keeps
   * its node and branch unknowns (it is never folded into a known node). */
  const double* src_ac;     /* [n_src] or NULL */
  /* parameter blocks of the CH_DEV_VA instances: per instance 2*n_params doubles — the module's parameters in
   * declaration order (defaults already applied, integers as doubles) followed by the $param_given flags */
  int64_t n_va_par;
  const double* va_par;     /* [n_va_par] or NULL */
} ch_desc;

/* Statistics — the fields CedarSim accumulates from NLStats/DEStats (src/dcop.jl:63-67,134-139) */
typedef struct ch_stats {
  int64_t nf;              /* residual (device) evaluations                     */
  int64_t njacs;           /* Jacobian evaluations                              */
  int64_t nfactors;        /* LU factorisations                                 */
  int64_t nsolve;          /* triangular solves                                 */
  int64_t nnonliniter;     /* Newton iterations (max over blocks, summed over samples: see DESIGN.md) */
  int64_t nnonlinconvfail; /* Newton convergence failures                       */
  int64_t naccept;         /* accepted time steps                               */
  int64_t nreject;         /* rejected time steps (LTE)                         */
  int64_t nrestarts;       /* DC random restarts used                           */
  double wall_seconds;     /* host wall-clock inside the call                   */
  double dc_seconds;       /* of which DC initialisation                        */
  double device_seconds;   /* sum of dominant-kernel durations measured with HIP events (0 for oracle) */
  int64_t n_kernel_launches;
  int64_t n_block_iters;   /* Newton iterations summed over every Jacobian block (exact work count) */
  int64_t n_step_attempts; /* time-step attempts (accepted + rejected + Newton failures)                */
  double barrier_seconds;  /* device-resident stepper: time one wave spent inside the grid-wide reductions (0 otherwise) */
  int32_t stepper;         /* which step controller ran: CH_STEPPER_HOST or CH_STEPPER_DEVICE (0 for DC-only calls) */
  int32_t stepper_mode;    /* device-resident stepper: CH_MODE_LOCKSTEP (one step sequence for the whole circuit / batch), CH_MODE_OWN_STEPS
                              (every independent block / sample its own sequence, output on the saveat grid), CH_MODE_BORDERED (coupled array
                              torn at its rail nodes: Schur complement on the border inside the kernel); 0 on the host stepper */
  /* the dominant kernel of the call, for roofline accounting: the time-stepping kernel(s) only, DC initialisation excluded */
  double step_kernel_seconds;    /* HIP-event time of those launches (device stepper: exact; host stepper: sampled launches, scaled) */
  int64_t step_kernel_launches;  /* their number (1 per transient on the device stepper, 1 per attempt on the host stepper)         */
  int64_t step_block_iters;      /* Newton iterations summed over blocks inside them                                               */
} ch_stats;

/* CedarDCOp options (src/dcop.jl:24-28, 53-94) */
typedef struct ch_dc_opts {
  double abstol;      /* residual inf-norm tolerance, default 1e-10 (dcop.jl:28)          */
  int32_t maxiters;   /* default 200 (dcop.jl:53)                                          */
  int32_t n_restarts; /* default 10 (num_trajectories, dcop.jl:53)                         */
  uint64_t seed;      /* RNG seed for u0 = 1e-7*randn (dcop.jl:60)                         */
  int32_t tran_mode;  /* 0: :dcop (sources at .dc), 1: :tranop (sources at tran(t=0))      */
  double dv_max;      /* Newton damping: max node-voltage change per iteration (0 = off)   */
  const double* x0;   /* optional initial guess [n_samples][n_mna] or NULL                 */
} ch_dc_opts;

/* transient options — solve(prob, IDA(); abstol, reltol) (src/sweeps.jl:456) */
typedef struct ch_tran_opts {
  double abstol;     /* default 1e-6 */
  double reltol;     /* default 1e-3 */
  int32_t max_order; /* 1..5 variable-order BDF, default 5 (IDA) */
  double dtmin;      /* default 1e-18*(t1-t0)... 0 = auto */
  double dtmax;      /* 0 = auto ((t1-t0)/10) */
  double dt0;        /* initial step, 0 = auto */
  int32_t max_steps; /* accepted steps before CH_ERR_MAXSTEPS (ReturnCode.MaxIters); 0 = 100 000, the default maxiters of solve(prob, IDA()) in Sundials.jl (the
                        reference passes none, src/sweeps.jl:456).  A transient that creeps (Newton failing whenever the step grows) ends there. */
  int32_t newton_maxiters; /* default 10 */
  int32_t n_saveat;        /* 0: save every accepted step (ONE step sequence and time vector for the whole circuit / batch) */
  const double* saveat;    /* [n_saveat] increasing times to save (dense output by interpolation).  With a saveat grid the samples of a batch,
                              and the structurally independent blocks of one circuit, may each take their own step sequence (what
                              sol(t) of separate solves would give; error control per sample / block) */
  ch_dc_opts dc;           /* initialisation (CedarDCOp) */
  int32_t skip_dc;         /* 1: start from dc.x0 as given (u0 passed by the caller, test/common.jl:36-43) */
  int32_t stepper;         /* CH_STEPPER_AUTO (default): device-resident controller where the circuit qualifies, host otherwise;
                              CH_STEPPER_HOST / CH_STEPPER_DEVICE force one (DEVICE fails with CH_ERR_UNSUPPORTED when it cannot run) */
  int32_t step_control;    /* CH_STEPS_AUTO (default): with a saveat grid, independent blocks / samples take their own steps under their
                              own error norm (above).  CH_STEPS_SHARED: ONE step sequence and ONE error norm over the whole circuit /
                              batch whatever the output grid — the answer of a single IDA() integrator over the whole system
                              (src/sweeps.jl:456), and the same controller a run without saveat uses: results of the two are then
                              comparable point for point */
} ch_tran_opts;

/* Where the sequential step controller of ch_tran runs (the policy is the same): on the host with one kernel
 * launch per step attempt, or inside ONE persistent cooperative launch per transient (blocks stay resident, the
 * accept/reject/order/step decision is taken from a grid-wide reduction by every wavefront identically). */
enum { CH_STEPPER_AUTO = 0, CH_STEPPER_HOST = 1, CH_STEPPER_DEVICE = 2 };
enum { CH_MODE_LOCKSTEP = 1, CH_MODE_OWN_STEPS = 2, CH_MODE_BORDERED = 3 };
enum { CH_STEPS_AUTO = 0, CH_STEPS_SHARED = 1 };

typedef struct ch_ctx ch_ctx;
typedef struct ch_circuit ch_circuit;
typedef struct ch_result ch_result;

typedef struct ch_info {
  int32_t n_nodes, n_branches, n_mna; /* MNA sizes of the description                          */
  int32_t n_unknowns;                 /* unknowns after structural simplification              */
  int32_t n_known;                    /* nodes eliminated as known (grounded-source chains)    */
  int32_t n_alias;                    /* nodes merged by 0 V ammeter sources                   */
  int32_t n_components;               /* independent diagonal blocks of the Jacobian           */
  int32_t max_component;              /* unknowns in the largest block                         */
  int32_t n_classes;                  /* structurally distinct blocks                          */
  int32_t n_mos, n_mos_classes;       /* MOS instances, distinct (model,geometry) classes      */
  int32_t path;                       /* 1 = fused block kernel, 2 = sparse level-scheduled    */
  int64_t nnz_jac, nnz_lu;            /* sparse path only                                      */
  int32_t n_samples;
} ch_info;

/* ---- defaults ---- */
void ch_dc_opts_default(ch_dc_opts*);
void ch_tran_opts_default(ch_tran_opts*);

/* ---- context: one per GPU.  Replaces: nothing in the reference (CPU only). ---- */
ch_ctx* ch_create(int device_id, char* err, size_t errlen);
void ch_destroy(ch_ctx*);
const char* ch_last_error(ch_ctx*);

/* ---- circuit: replaces CircuitIRODESystem(circuit) + DAEProblem(sys, …) construction
 *      (src/circuitodesystem.jl:147-164, src/sweeps.jl:444): structural analysis done once. ---- */
ch_circuit* ch_circuit_build(ch_ctx*, const ch_desc*);
void ch_circuit_free(ch_circuit*);
int ch_circuit_info(ch_circuit*, ch_info*);
/* Result of the structural analysis, for host mirrors and tests: for node 0..n_nodes the index of
 * the unknown that carries its voltage (or -1) and of the known value (or -1); for each MNA branch
 * the unknown of its current (or -1 when the source was eliminated). */
int ch_circuit_maps(ch_circuit*, int32_t* node_unknown, int32_t* node_known, int32_t* branch_unknown);

/* ---- samples: replaces remake(prob, p=sim) over the sweep (src/sweeps.jl:471-482). ----
 * values is slot-major: values[slot_i * (sample_hi-sample_lo) + (s - sample_lo)]. */
int ch_set_samples(ch_circuit*, int32_t n_samples);
int ch_set_params(ch_circuit*, int32_t sample_lo, int32_t sample_hi, int32_t n_slots,
                  const int32_t* slot_ids, const double* values);

/* ---- DC operating point: replaces initialize_dae!(…, ::CedarDCOp) + bootstrapped_nlsolve
 *      (src/dcop.jl:53-94,157-200).  x_out: [n_samples][n_mna]. status_out: [n_samples] or NULL. ---- */
int ch_dc(ch_circuit*, const ch_dc_opts*, double* x_out, int32_t* status_out, ch_stats* stats);

/* ---- transient: replaces solve(prob, IDA(); abstol, reltol, initializealg=CedarDCOp())
 *      (src/sweeps.jl:456, test/gf180_dff.jl:25). ---- */
int ch_tran(ch_circuit*, double t0, double t1, const ch_tran_opts*, ch_result** out);

int64_t ch_result_n_times(const ch_result*);
const double* ch_result_times(const ch_result*);  /* [n_times]                                  */
const double* ch_result_values(const ch_result*); /* [n_obs][n_times][n_samples]                */
/* Dense output of a run WITHOUT a saveat grid (`sol(t, idxs=…)`, test/gf180_dff.jl:29-33): entry i is the number m of newest
 * saved points, row i included, through which the polynomial of the step that ended at times[i] runs — for t in
 * (times[i-1], times[i]] the solution is the Lagrange interpolant through rows i-m+1 .. i, which is what a saveat grid would
 * have returned there.  0: no polynomial for this row (the initial state; every row of a run on a saveat grid).  [n_times] */
const int32_t* ch_result_dense_points(const ch_result*);
/* The values of ch_result_values STILL IN HBM, same layout [n_obs][n_times][n_samples], for a device-side consumer — the result gather of
 * a sharded sweep (src/sweeps.jl:471-502 collects the per-point solutions on the host; here RCCL moves the rows GPU to GPU).  *ptr is a
 * device pointer on the context's GPU, owned by the circuit and valid until the next call on that circuit or ch_circuit_free.
 * CH_ERR_UNSUPPORTED (and *ptr = NULL) when the rows are not kept: the host stepper ran, the row buffer was drained in batches, or an
 * observable is a known node / merged node / eliminated branch (those are filled in on the host). */
int ch_result_device_values(const ch_result*, const double** ptr, int64_t* n_doubles);
const double* ch_result_final_state(const ch_result*); /* [n_samples][n_mna] at the last time   */
int ch_result_stats(const ch_result*, ch_stats*);
int ch_result_status(const ch_result*);           /* CH_OK or CH_ERR_*                          */
void ch_result_free(ch_result*);

/* ---- one residual/Jacobian evaluation: replaces prob.f.f(out,du,u,p,t) and
 *      prob.f.jac(J,du,u,p,γ,t) (benchmarks/benchmark_common.jl:138,155).
 *      Evaluates on the GPU at x_mna for sample `sample`:
 *        F = i(x,t) + alpha0*q(x)   (history term excluded),  Q = q(x),
 *        J = di/dx + alpha0*dq/dx as dense row-major [n_mna*n_mna] (rows/cols of eliminated
 *        unknowns are returned as identity rows so the matrix stays usable by a host LU).
 *      mode: 0 = :dcop source values, 1 = :tran source values at t. ---- */
int ch_eval(ch_circuit*, int32_t sample, const double* x_mna, double t, double alpha0, int32_t mode,
            double* F_out, double* Q_out, double* J_out);

/* ---- BSIM4 device evaluation only (roofline kernel): evaluates every MOS instance at the
 *      given terminal voltages.  v: [n_mos][4] (d,g,s,b); out: [n_mos][40] =
 *      {i[4], q[4], g[16], c[16]} per instance.  Used by the parity tests and bench. ---- */
int ch_mos_eval(ch_circuit*, int32_t sample, const double* v, double* out);
/* Same result computed the way the Newton kernel does it: four lanes per instance, one partial
 * derivative per lane, columns exchanged with quad shuffles. */
int ch_mos_eval_quad(ch_circuit*, int32_t sample, const double* v, double* out);

/* ---- names of BSIM4 parameters (for host-side card parsing) ---- */
int32_t ch_bsim4_npar(void);
const char* ch_bsim4_param_name(int32_t idx);
int32_t ch_bsim4_param_ignored(const char* name); /* 1 if accepted-and-ignored */

/* ---- small-signal AC analysis.  Replaces: ac!(circ) + freqresp(ac, sym, ωs) (src/ac.jl:166-177, 75-102,
 * 267-284): DC operating point with CedarDCOp, linearisation A = ∂F/∂u, E = mass matrix, B = ∂F/∂ϵω, then
 * C·(jωE − A)⁻¹·B per frequency.  Here: G = ∂i/∂x and C = ∂q/∂x from the same device kernels at the DC
 * point, and one batched complex LU (G + jωC)·x = b per (block, sample, frequency) on the GPU.
 * freqs_hz[n_freq]; x_ac_out[n_samples][n_freq][n_mna][2] (re, im) in MNA order, like ch_dc's x_out
 * (eliminated branch currents are NaN; nodes tied to ground through non-AC sources are 0).  A circuit on the sparse path is
 * taken as one dense block per sample and may have up to 4096 unknowns (CH_ERR_UNSUPPORTED above that). ---- */
int ch_ac(ch_circuit*, const ch_dc_opts*, int32_t n_freq, const double* freqs_hz, double* x_ac_out, ch_stats* stats);

/* ---- output-noise PSD.  Replaces: noise!(circ) + PSD(noise, sym, ωs) (src/ac.jl:136-163, 178-186, 286-305).
 * Noise sources built: resistor thermal noise, 4kT/R per instance (src/simpledevices.jl:72-76), T = temp + 273.15, and the
 * white / flicker sources of compiled Verilog-A modules (BSIM-CMG: test/ac.jl:155-237).  In THIS call CH_DEV_MOS devices enter with
 * their small-signal conductances and capacitances only and contribute no noise power of their own — the PSD is that of the
 * resistors and compiled devices seen through the MOSFETs.  The BSIM4 functor's own sources (channel thermal and flicker noise,
 * test/inverter_noise.jl:56-124) are opt-in: ch_noise_ex below with mos_noise = 1.
 * out_kind/out_index select the observed unknown like ch_desc.obs_kind/obs_index (0 = node voltage, 1 = branch
 * current); psd_out[n_samples][n_freq] in V²/Hz (A²/Hz), computed with one adjoint solve per frequency. ---- */
int ch_noise(ch_circuit*, const ch_dc_opts*, int32_t out_kind, int32_t out_index, int32_t n_freq, const double* freqs_hz,
             double* psd_out, ch_stats* stats);

/* ---- output noise with the BSIM4 MOSFETs' own sources, and per-source contributions (ngspice: the per-device lines of .noise).
 * ch_set_mos_noise hands the noise parameters of model card `model` (index into ch_desc.model_par's cards): par[CH_B4N_NPAR], NaN = not
 * given (BSIM4.5 default of the device type).  A model that got no row runs on the defaults.
 * ch_noise_ex is ch_noise with options.  mos_noise != 0: every CH_DEV_MOS of the output block adds, between its drain and its source
 * and times its multiplier, (1) channel thermal noise of tnoimod 0, 4kT ntnoi ueff|Qinv| / (Leff^2 + ueff|Qinv| Rds), Qinv the
 * inversion charge of the capMod-2 half, and (2) flicker noise with exponent ef: fnoimod 0, kf |Ids|^af / (coxe Leff^2), or fnoimod 1
 * (the default), the unified model of the BSIM4.5.0 manual 9.1 with lintnoi = 0.  CH_ERR_UNSUPPORTED, with the model card named in
 * ch_last_error: tnoimod 1 (the holistic model's correlated source-side noise voltage does not fit a one-port source table), an
 * fnoimod outside 0 / 1, a card without an intrinsic charge model.  Not built: gate-current shot noise, the thermal noise of rsh
 * source / drain resistors (the engine has neither).  The derivatives of the PSD: ch_noise_sens below.
 * contrib_out, or NULL: [n_samples][n_freq][n_src], every column of the source table's share |y_a - y_b|^2 pwr / f^ex of psd_out;
 * n_src and the meaning of a column from ch_noise_sources.  With mos_noise = 0 and contrib_out = NULL the call is ch_noise, bit for bit. ---- */
typedef struct ch_noise_opts {
  int32_t mos_noise; /* 0: ch_noise's sources only; 1: the MOSFETs' too */
} ch_noise_opts;
int ch_set_mos_noise(ch_circuit*, int32_t model, const double* par /* [CH_B4N_NPAR] */);
int ch_noise_ex(ch_circuit*, const ch_dc_opts*, const ch_noise_opts*, int32_t out_kind, int32_t out_index, int32_t n_freq,
                const double* freqs_hz, double* psd_out, double* contrib_out /* may be NULL */, ch_stats* stats);
/* The source table of the block that holds the output.  Its columns are fixed by the structure: one per resistor, two per MOSFET
 * (thermal, flicker; power 0 in an analysis without mos_noise), 16 per compiled Verilog-A instance (unused ones have power 0), in
 * device order.  With every array NULL the call only counts them into *n_src (no analysis needed).  Otherwise it reports sample
 * `sample` of the table the last ch_noise_ex (with mos_noise or a contributions buffer) built for this output: dev[n_src] the device
 * of ch_desc, a[n_src] / b[n_src] the MNA indices of the two terminals (-1: ground or a node held by sources), pwr[n_src] in A^2/Hz
 * at 1 Hz, ex[n_src] the exponent of 1/f (0 = white), and mos_operands[n_src][CH_B4N_NOPERAND] or NULL, for a MOSFET's columns
 * the operand row its records were formed from — ids ueff vgsteff abulk vdseff vds rds esat litl leff weff*nf coxe cdep0 cit vtm
 * qinv, mode frame — and zeros elsewhere.  An output held by ideal sources has no table: *n_src = 0. ---- */
int ch_noise_sources(ch_circuit*, int32_t out_kind, int32_t out_index, int32_t sample, int32_t* n_src, int32_t* dev, int32_t* a,
                     int32_t* b, double* pwr, double* ex, double* mos_operands /* may be NULL */);

/* ---- DC parameter sensitivities, direct method.  Replaces: the forward sensitivities the reference obtains by differentiating
 * through its solve with SciMLSensitivity (test/sensitivity.jl: d/dp of the two-resistor divider's node voltage).  Here the
 * circuit is a function of its declared slots: F(x, p) = 0 at the operating point gives G · dx/dp_k = -dF/dp_k, with G = di/dx from
 * the linearisation ch_ac uses and dF/dp_k from two residual evaluations at the FIXED operating point in which only the table the
 * slot reaches is perturbed (no second Newton solve; the circuit's tables are left bit for bit as they were).  One real dense LU
 * per (block, sample) on the GPU, all requested parameters as right-hand sides.
 * slot_ids[n_par] index ch_desc.slot_*; any declared slot, whether ch_set_params gave it per-sample values or not (then it is
 * differentiated at its base value).  Every sample of ch_set_samples is differentiated at its own parameter point.
 * Step of the difference: slots the residual is linear in (CH_SLOT_DEV_MULT, the gain of a VCVS / VCCS, CH_SLOT_GMIN unless a
 * compiled Verilog-A instance is present, and CH_SLOT_SRC_DC / _SRC_PAR unless the source sets a known node that a MOSFET or compiled
 * device sits on) take a forward difference with an absolute step (1; 2^-20 S for gmin), exact up to rounding at any p;
 * everything else a central difference with h = rel_step*|p| (h = rel_step at p = 0).  DESIGN.md 2.7b.
 * x_out [n_samples][n_mna] or NULL: the operating point, as ch_dc returns it.  sens_out [n_samples][n_par][n_mna] = d x_mna / d p_k
 * in MNA order: a known (eliminated) node carries the exact derivative of its known-value expression (the sum of its coefficients
 * of the slot's source; 0 for other slots), a node merged by a 0 V ammeter its representative's row, an eliminated branch current
 * CH_NAN.  status_out [n_samples] or NULL: a sample whose operating point failed has its ch_dc status there and NaN rows; the other
 * samples are still served and the call returns the operating point's code.  CH_ERR_INVALID: bad slot id or n_par < 1;
 * CH_ERR_SINGULAR: a block's G does not factor; CH_ERR_UNSUPPORTED above 4096 unknowns on the sparse path, like ch_ac.
 * ch_stats: dc_seconds = the operating point (host wall); step_kernel_seconds / step_kernel_launches = the residual evaluations behind
 * it (HIP events, sampled like every Newton launch); device_seconds = all of those launches plus the solve kernel's event time. ---- */
typedef struct ch_sens_opts {
  double rel_step;        /* default 2^-17: h = rel_step*|p| for slots whose residual is not linear in p */
  const double* abs_step; /* [n_par] or NULL; an entry > 0 replaces the step of that parameter (the kind of difference stays) */
} ch_sens_opts;
void ch_sens_opts_default(ch_sens_opts*);
int ch_dc_sens(ch_circuit*, const ch_dc_opts*, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* /* NULL = defaults */,
               double* x_out, double* sens_out, int32_t* status_out, ch_stats* stats);

/* ---- AC parameter sensitivities, direct method: the derivative of the small-signal solution of ch_ac with respect to declared slots
 * (ngspice: .sens ... ac).  With Y = G + jwC and Y x = b at the operating point xop(p):  Y dx/dp_k = -(dY/dp_k) x, where
 * dY/dp_k = (explicit) dY/dp_k at fixed xop  +  (state) sum_j dY/dx_j * dxop_j/dp_k.  The explicit part is a difference of the G, C
 * of the very perturbed evaluations ch_dc_sens makes (same slots, same step rule, same ch_sens_opts); the state part — the bias shift:
 * moving a load resistor or a supply moves gm and gds — a central difference of G, C at xop +- eps_k * dxop/dp_k with the circuit's own
 * tables, eps_k such that the largest node-voltage shift is rel_step * 1 V.  It is skipped where dxop/dp_k is zero on every node and in
 * circuits without a MOSFET or compiled Verilog-A instance (G, C do not depend on x there).  db/dp_k = 0: |ac| is not a slot and a
 * source's DC value does not enter b.  One complex LU per (frequency, block, sample) serves all parameters; no second Newton solve.
 * x_ac_out [n_samples][n_freq][n_mna][2] or NULL: what ch_ac returns.  dc_sens_out [n_samples][n_par][n_mna] or NULL: what ch_dc_sens
 * returns.  sens_out [n_samples][n_freq][n_par][n_mna][2] = d x_ac / d p_k (re, im) in MNA order: a known node carries no small
 * signal (0), a node merged by a 0 V ammeter its representative's row, an eliminated branch current CH_NAN.  status_out as in
 * ch_dc_sens: a sample whose operating point failed has NaN rows and its status, the others are served.  CH_ERR_INVALID: bad slot id,
 * n_par < 1, n_freq < 1, a negative or non-finite frequency, sens_out NULL; CH_ERR_SINGULAR: a G or a G + jwC does not factor (NaN for
 * that system only); CH_ERR_UNSUPPORTED above 4096 unknowns on the sparse path, and for the one slot that moves b: the multiplier
 * of an AC-driven current source.  Nothing writes the circuit's tables or the
 * operating point.  DESIGN.md 2.7c. ---- */
int ch_ac_sens(ch_circuit*, const ch_dc_opts*, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* /* NULL = defaults */,
               int32_t n_freq, const double* freqs_hz, double* x_ac_out, double* dc_sens_out, double* sens_out,
               int32_t* status_out, ch_stats* stats);

/* ---- noise PSD parameter sensitivities, direct method on the adjoint system: the derivative of the output PSD of ch_noise /
 * ch_noise_ex with respect to declared slots.  With Y = G + jwC, the adjoint solve Y^T y = e_out and the source table of the output
 * block (entries e between the unknowns a_e and b_e, power pwr_e, exponent ex_e):
 *     S(f) = sum_e |dy_e|^2 pwr_e / f^ex_e,   dy_e = y[a_e] - y[b_e]
 *     Y^T dy_k = -(dY/dp_k)^T y
 *     dS/dp_k  = sum_e [ 2 Re(conj(dy_e) d(dy)_{k,e}) pwr_e + |dy_e|^2 dpwr_{k,e} ] / f^ex_e
 * dY/dp_k and dpwr_k are total derivatives: the explicit part at the fixed operating point (a difference of G, C and of the source
 * table built with the perturbed tables of ch_dc_sens: same slots, same step rule, same ch_sens_opts) plus the bias shift (a central
 * difference of both at xop +- eps_k * dxop/dp_k with the circuit's own tables, under the conditions of ch_ac_sens).  A resistor's
 * thermal noise moves only explicitly (R, its multiplier, temp); a MOSFET's records move explicitly with w, l, card entries and
 * temp and with everything else through the bias.  Terminals and exponents do not move with any built-in slot; a compiled Verilog-A
 * module whose flicker exponent follows the slot is refused with CH_ERR_UNSUPPORTED, the slot named in ch_last_error.  One transposed
 * complex LU per (frequency, sample) of the output block serves y and all parameters; no second Newton solve.
 * The ch_noise_opts (NULL = ch_noise's sources) act as in ch_noise_ex, refusals included.  psd_out [n_samples][n_freq]: the bits of
 * ch_noise / ch_noise_ex.  dpsd_out [n_samples][n_freq][n_par] = dS/dp_k.  dc_sens_out [n_samples][n_par][n_mna] or NULL: what ch_dc_sens
 * returns.  An output held by ideal sources gives zeros for every sample that has an operating point.  status_out as in ch_dc_sens: a sample whose operating point failed
 * has NaN rows and its status, the others are served.  CH_ERR_INVALID, before the DC solve: bad slot id, n_par < 1, n_freq < 1, a
 * negative or non-finite frequency, psd_out or dpsd_out NULL; CH_ERR_SINGULAR: a G or a Y^T does not factor (NaN for that system only);
 * CH_ERR_UNSUPPORTED above 4096 unknowns on the sparse path.  Nothing writes the circuit's tables or the operating point.
 * DESIGN.md 2.7f. ---- */
int ch_noise_sens(ch_circuit*, const ch_dc_opts*, const ch_noise_opts* /* NULL = ch_noise's sources */, int32_t n_par,
                  const int32_t* slot_ids, const ch_sens_opts* /* NULL = defaults */, int32_t out_kind, int32_t out_index,
                  int32_t n_freq, const double* freqs_hz, double* psd_out /* [S][n_freq] */, double* dpsd_out /* [S][n_freq][n_par] */,
                  double* dc_sens_out /* may be NULL */, int32_t* status_out, ch_stats* stats);

/* ---- compiled Verilog-A modules.  Replaces: the device functors `make_spice_device` generates from a
 * parsed module (src/vasim.jl:649-867).  Modules are compiled ahead of time into the library by
 * cedarsim.jl_amd/va (front-end + code generator) — the counterpart of the reference's precompiled model
 * packages (src/ModelLoader.jl).  ch_va_eval evaluates one module instance on the GPU at given node voltages:
 * st[144] = [I(8) | Q(8) | dI/dV (8x8) | dQ/dV (8x8)] (stamp-level parity entry point, like ch_mos_eval). ---- */
int32_t ch_va_n_modules(void);
int32_t ch_va_find(const char* module_name);                                  /* id or -1 */
const char* ch_va_module_name(int32_t id);
int32_t ch_va_module_info(int32_t id, int32_t* n_ports, int32_t* n_nodes, int32_t* n_params);
const char* ch_va_node_name(int32_t id, int32_t k);
const char* ch_va_param_name(int32_t id, int32_t k);
int ch_va_eval(ch_ctx*, int32_t id, const double* par_and_given, const double* v_nodes, double temperature_k, double gmin,
               double* st_out);
/* Operating-point observables of a module: the variables declared with a (* desc = "..." *) attribute
 * (src/vasim.jl:742-753, 841-843: `observed!(var, DScope(dscope, name))`), evaluated on the GPU at given node voltages. */
int32_t ch_va_n_opvars(int32_t id);
const char* ch_va_opvar_name(int32_t id, int32_t k);
int ch_va_opvars(ch_ctx*, int32_t id, const double* par_and_given, const double* v_nodes, double temperature_k, double gmin,
                 double* op_out);

/* ---- library/kernel introspection ---- */
const char* ch_version(void);

/* ---- measurement utility ("report against ... the builder's own measured STREAM-triad").
 * a[i] = b[i] + s*c[i] over three fp64 arrays of n_doubles each, `iters` timed passes after one warm-up;
 * returns the best pass in GB/s (24 bytes per element) in *gbps_out.  No reference counterpart. ---- */
int ch_bench_triad(ch_ctx*, int64_t n_doubles, int32_t iters, double* gbps_out);
/* Vector fp64 FMA peak of this GPU, measured: 16 independent v_fma_f64 chains per lane, 8 waves per SIMD;
 * best of `iters` passes in TFLOP/s (the eval kernel's fp64 rate is reported against this). */
int ch_bench_fp64(ch_ctx*, int32_t iters, double* tflops_out);

/* ---- test hook: fill the LDS of every CU with a NaN / negative-integer pattern (LDS keeps what the previous kernel left; a
 * kernel that reads LDS it did not stage must not get away with a fresh process's zeros).  No reference counterpart. ---- */
int ch_debug_poison_lds(ch_ctx*);
/* Test hook: y[i] = f(x[i]) with the DEVICE's own fp64 functions (hardware seeds + polynomial / Newton steps instead of the library
 * sequences: cedarsim.jl_amd/csrc/va_rt.hpp, ch_bsim4.hpp) — which = 0: exp as compiled Verilog-A code calls it, 1: ln likewise
 * (incl. the special values), 2: the ln of the BSIM4 device code.  Host arrays of n doubles. */
int ch_debug_math(ch_ctx*, int32_t which, int32_t n, const double* x, double* y);

/* ---- Transient parameter sensitivities, direct method.  Replaces: the ODEForwardSensitivityProblem of test/sensitivity.jl
 * (d v(t)/d R along the waveform).  ch_tran on the host stepper, with the same launches and arguments for the state, plus at every
 * accepted step to t_{n+1} — where f(x, t, p) + a0 q(x, p) + sum_j a_j q_j = 0 was solved — one linear solve per (block, sample)
 * for all parameters:   (G + a0 C) s_k = -[ df/dp_k + a0 dq/dp_k + sum_j a_j w_{j,k} ],   w_{n+1,k} = C s_k + dq/dp_k,
 * s_k = d x_{n+1} / d p_k, w_{j,k} = d q_j / d p_k a second history ring beside the charges.  G, C from one evaluation at the
 * accepted state, the partials from differences of perturbed evaluations there (slots, step rule and ch_sens_opts of ch_dc_sens;
 * the perturbed tables are built once per transient).  The step sequence is held fixed: the sensitivities take no part in the
 * error test or in step and order selection, so the result is the derivative of the DISCRETE solution on the steps the run took.
 * It converges to the continuous sensitivity with the tolerances; it is not what differencing two adaptive runs gives.
 * Start: s_0 = the DC sensitivities at the transient's own operating point (0 with skip_dc), w_0 = C s_0 + dq/dp at t0.
 * A slot that moves a break point (td, tr, tf, pw, period of a PULSE) is refused with CH_ERR_UNSUPPORTED naming the slot;
 * so is stepper = CH_STEPPER_DEVICE (AUTO means the host stepper here) and, like ch_ac, more than 4096 unknowns on the sparse
 * path.  CH_ERR_INVALID: bad slot id, n_par < 1, or what ch_tran refuses.  CH_ERR_SINGULAR: a G + a0 C did not factor (NaN rows
 * from that step on).  The result is a ch_tran result (times, dense points, values, final state, statistics: nf counts the extra
 * evaluations, nfactors / nsolve the extra solves, n_kernel_launches the extra launches) that also carries the sensitivity rows:
 * ch_result_sens = d(observable)/d p_k as [n_obs][n_par][n_times][n_samples], on a saveat grid interpolated with the weights the
 * state rows use.  An observable merged with another takes its primary's rows, a known node the exact derivative of its value
 * expression at each saved time, an eliminated branch current CH_NAN.  DESIGN.md 2.7d. ---- */
int ch_tran_sens(ch_circuit*, double t0, double t1, const ch_tran_opts*, int32_t n_par, const int32_t* slot_ids,
                 const ch_sens_opts* /* NULL = defaults */, ch_result** out);
int32_t ch_result_n_par(const ch_result*);        /* 0 for a result of ch_tran */
const double* ch_result_sens(const ch_result*);   /* [n_obs][n_par][n_times][n_samples], NULL for a result of ch_tran */

/* ---- waveform measurements over a finished transient (.measure), one value per (measure, sample), on the GPU, with exact derivatives
 * of the discrete measure with respect to the rows.  The definitions are in csrc/ch_measure_host.hpp and DESIGN.md 2.7e.
 * A signal is y_i = scale * (V[row_a][i] - V[row_b][i]); row_b = -1: no second row.  Between rows the signal is the run's own
 * dense-output polynomial (the rows ch_result_dense_points names), a line where there is none (every saveat grid).
 *   WHEN       s1: the time of the count-th event (count >= 1, or CH_MEAS_LAST) of `edge` against `level` at or after td
 *   DELAY      s1: trig event, s2: targ event; t_targ - t_trig
 *   FIND_WHEN  s1: the event, s2: the signal read at its time
 *   FIND_AT    s1 at time `at`
 *   INTEG AVG RMS MIN MAX PP   s1 over [from, to] clipped to the run (trapezoid rule on from, the rows strictly inside, to)
 * status: 0 ok; 1 event not found; 2 empty window; 3 a non-finite row in the span the measure read; 4 event found on a flat
 * interpolant (value fine, sensitivities NaN).  The value is CH_NAN for 1..3; a failed measure never fails the call. */
enum { CH_MEAS_WHEN = 0, CH_MEAS_DELAY, CH_MEAS_FIND_WHEN, CH_MEAS_FIND_AT, CH_MEAS_INTEG, CH_MEAS_AVG, CH_MEAS_RMS, CH_MEAS_MIN, CH_MEAS_MAX, CH_MEAS_PP, CH_MEAS_N_KINDS };
enum { CH_EDGE_RISE = 1, CH_EDGE_FALL = 2, CH_EDGE_CROSS = 3 };
#define CH_MEAS_LAST (-1)
typedef struct ch_measure_side {
  int32_t row_a, row_b;  /* rows of the signal; row_b = -1: none */
  double scale;
  double level;
  int32_t edge, count;   /* CH_EDGE_*; n >= 1 or CH_MEAS_LAST */
  double td;             /* events before td do not count */
} ch_measure_side;
typedef struct ch_measure_spec {
  int32_t kind, reserved;
  ch_measure_side s1, s2;
  double at, from, to;
} ch_measure_spec;
/* Measures of any rows: values [n_rows][n_times][n_samples] (host), times [n_times] non-decreasing, dense_points [n_times] or NULL
 * (all lines), sens [n_rows][n_par][n_times][n_samples] or NULL with n_par = 0.  out_value / out_status [n_meas][n_samples],
 * out_sens [n_meas][n_par][n_samples] or NULL.  CH_ERR_INVALID, before anything is uploaded and with the measure named in
 * ch_last_error: a row out of range, count 0, a non-finite level, an unknown kind or edge, out_sens without sens. */
int ch_measure_rows(ch_ctx*, int64_t n_times, const double* times, const int32_t* dense_points, int32_t n_rows, int32_t n_samples,
                    const double* values, int32_t n_par, const double* sens, int32_t n_meas, const ch_measure_spec* specs,
                    double* out_value, double* out_sens, int32_t* out_status);
/* The same over a result of ch_tran / ch_tran_sens; rows are observable indices.  The rows are read in HBM where the circuit still
 * holds them (ch_result_device_values; the result must then be measured before the next call on its circuit), else the rows the
 * specs name are uploaded.  out_sens needs a result of ch_tran_sens: [n_meas][ch_result_n_par][n_samples].
 * Lifetime: the result keeps a pointer to the context of the circuit that made it and launches on its stream, so that context must
 * still be alive; a result for which ch_result_device_values succeeds also reads the circuit's own buffer, so the circuit must be
 * alive and untouched since the transient (no other call on it, no ch_circuit_free).  A result measured later than that must come
 * from a run whose rows were not kept on the device (ch_result_device_values fails): it carries its rows itself. */
int ch_result_measure(const ch_result*, int32_t n_meas, const ch_measure_spec* specs, double* out_value, double* out_sens, int32_t* out_status);

/* ---- frequency-domain measurements (.measure ac / noise), one value per (measure, sample), on the GPU, with exact derivatives of the
 * discrete measure with respect to the rows.  The definitions are in csrc/ch_fmeasure_host.hpp and DESIGN.md 2.7g.
 * Rows are complex: H_i = scale * (X[row_a][i] - X[row_b][i]) as (re, im); row_b = -1: no second row; a real quantity (a PSD) has im = 0.
 * A side reads the real signal g = `sig`(H): RE, IM, MAG, DB = 20 log10 |H|, DB10 = 10 log10 re, PHASE in degrees, unwrapped along the
 * grid from row 0 (phi_i = atan2(im_i, re_i) + 360 k_i, k the running count of steps whose raw increment leaves (-180, 180]).
 * Between rows g is the line in (u, g), u = log10 f (CH_FX_LOG) or f (CH_FX_LIN).
 *   WHEN       s1: the frequency (Hz) of the count-th event (count >= 1, or CH_MEAS_LAST) of `edge` against the level at or after fd;
 *              the level is `level`, or level + g(ref_at) when ref_at is finite (the signal's own interpolated value there)
 *   FIND_WHEN  s1: the event, s2: the signal read at its frequency
 *   FIND_AT    s1 at frequency `at`
 *   INTEG AVG RMS MIN MAX PP   s1 over [from, to] clipped to the grid (trapezoid rule in linear f on from, the rows strictly inside, to)
 * Event rules, status 0..4 and the NaN values are those of ch_measure_spec; a signal that is not finite at a row the measure reads
 * (|H| = 0 under DB or PHASE) is status 3; status 5 (ch_ac_measure only): the sample has no operating point. */
enum { CH_FMEAS_WHEN = 0, CH_FMEAS_FIND_WHEN, CH_FMEAS_FIND_AT, CH_FMEAS_INTEG, CH_FMEAS_AVG, CH_FMEAS_RMS, CH_FMEAS_MIN, CH_FMEAS_MAX, CH_FMEAS_PP, CH_FMEAS_N_KINDS };
enum { CH_FSIG_RE = 0, CH_FSIG_IM, CH_FSIG_MAG, CH_FSIG_DB, CH_FSIG_DB10, CH_FSIG_PHASE, CH_FSIG_N };
enum { CH_FX_LIN = 0, CH_FX_LOG = 1 };
typedef struct ch_fmeasure_side {
  int32_t row_a, row_b;  /* rows of the signal; row_b = -1: none */
  double scale;
  int32_t sig, edge;     /* CH_FSIG_*; CH_EDGE_* */
  double level;
  double ref_at;         /* finite: the level is relative to g(ref_at); CH_NAN or infinite: absolute */
  int32_t count, reserved;   /* n >= 1 or CH_MEAS_LAST */
  double fd;             /* events below fd do not count */
} ch_fmeasure_side;
typedef struct ch_fmeasure_spec {
  int32_t kind, xscale;  /* CH_FMEAS_*; CH_FX_* */
  ch_fmeasure_side s1, s2;
  double at, from, to;
} ch_fmeasure_spec;
/* Measures of any host rows: freqs_hz [n_freq] finite and strictly increasing (all > 0 when a spec asks for CH_FX_LOG), values
 * [n_rows][n_freq][n_samples][2], sens [n_rows][n_par][n_freq][n_samples][2] or NULL with n_par = 0.  out_value / out_status
 * [n_meas][n_samples], out_sens [n_meas][n_par][n_samples] or NULL.  Only the rows the specs name are uploaded.  CH_ERR_INVALID, before
 * anything is uploaded and with the measure's index in ch_last_error, for an invalid spec. */
int ch_freq_measure_rows(ch_ctx*, int32_t n_freq, const double* freqs_hz, int32_t n_rows, int32_t n_samples, const double* values,
                         int32_t n_par, const double* sens, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value,
                         double* out_sens, int32_t* out_status);
/* The AC analysis measured where it lies: the launches of ch_ac (n_par = 0) or of ch_ac_sens, then a gather of the MNA rows the specs
 * name and one measure kernel on the same stream; only out_value / out_status [n_meas][n_samples] and out_sens [n_meas][n_par][n_samples]
 * come back.  Rows are MNA indices (a known node is 0, a merged node its representative, an eliminated branch current CH_NAN).
 * sample_status [n_samples] or NULL as status_out of ch_ac_sens; a sample without an operating point has status 5 and NaN in every
 * measure.  Refusals are those of ch_ac_sens (of ch_ac with n_par = 0); an invalid spec is refused before the DC solve. */
int ch_ac_measure(ch_circuit*, const ch_dc_opts*, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* /* NULL = defaults */,
                  int32_t n_freq, const double* freqs_hz, int32_t n_meas, const ch_fmeasure_spec* specs, double* out_value,
                  double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats);

/* ---- loop-gain (stability) analysis of a closed loop, the bias kept: Tian's loop gain at a voltage-source probe `vprobe x y` (DC value
 * normally 0) inserted in the loop wire, terminal x (+) facing the side the loop signal arrives from, y (-) the side it goes into.  Two
 * excitations of Y(w) = G + jwC at the operating point: the probe at 1 V (keep V2 = v_x) and a unit current into x with the probe at
 * 0 V (keep I1, the probe's branch current from x through it to y); u = V2 - I1, T = u / (1 - u).  The reversed probe measures the
 * reverse loop gain, so the direction matters.  The description must carry |ac| = 1 on the probe's source and 0 on every other one
 * (an AC-driven voltage source is never folded or merged).  T_out [S][n_freq][2] or NULL; with n_par slots dT_out
 * [S][n_freq][n_par][2] (or NULL) = (du/dp) / (1 - u)^2, du/dp from two adjoint vectors and the dY/dp of ch_ac_sens: no per-parameter
 * solve.  Measures as ch_ac_measure, over one row: 0 = T; out_value / out_status [n_meas][S], out_sens [n_meas][n_par][S].  A sample
 * without an operating point has its status in sample_status, NaN rows and measure status 5; the others are served.  1 - u = 0 is no
 * failure (what IEEE gives).  Refused before the DC solve, with the probe named in ch_last_error: probe_dev is no voltage source; its
 * + node is ground or held by ideal sources; its branch current was eliminated; a slot is the probe's own multiplier
 * (CH_ERR_UNSUPPORTED); more than 4096 coupled unknowns (CH_ERR_UNSUPPORTED); an invalid spec.  DESIGN.md 2.7i. */
int ch_loop_gain(ch_circuit*, const ch_dc_opts*, int32_t probe_dev, int32_t n_par, const int32_t* slot_ids, const ch_sens_opts* /* NULL = defaults */,
                 int32_t n_freq, const double* freqs_hz, double* T_out, double* dT_out, int32_t n_meas, const ch_fmeasure_spec* specs /* rows: 0 = T */,
                 double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats);

/* ---- N-port network analysis: the S, Y and Z parameters of the circuit seen from n_ports (1 .. 8) independent voltage sources
 * `vpJ a b`, numbered 1 .. P in the order of port_devs (device indices), the bias kept: a port's DC value stays, so a port may bias
 * a gate.  Y(w) = G + jwC at the operating point; run k puts 1 V AC on port k and 0 V on the others, which stay ideal sources (AC
 * shorts).  A source's branch current flows from + through the source to -, so the current entering the network at port j is -i_pj:
 * Yp[j][k] = -x_k[row of i_pj].  With the real, finite, positive reference impedances z0[P] and y = sqrt(z0) Yp sqrt(z0):
 * S = (I - y)(I + y)^-1, Z = Yp^-1.  The description must carry |ac| = 1 on every port's source and 0 on every other one (an
 * AC-driven voltage source is never folded or merged); the ports' multipliers must be 1.  One factorisation of Y per (frequency,
 * sample) serves all P columns.  S_out, Y_out, Z_out: [S][n_freq][P][P][2] or NULL, entry [j][k] the response at port j to port k.
 * With n_par slots dS_out, dY_out, dZ_out: [S][n_freq][n_par][P][P][2] or NULL, from P adjoint vectors Y^T l_j = e_(row of i_pj)
 * and the dY/dp of ch_ac_sens (bias shift included): dYp[j][k]/dp = l_j^T (dY/dp) x_k, dS = -1/2 (I + S)(sqrt(z0) dYp sqrt(z0))(I + S),
 * dZ = -Z dYp Z; no per-parameter solve.  Measures as ch_ac_measure, over the rows kind * P^2 + j * P + k with kind 0 = S, 1 = Y,
 * 2 = Z; out_value / out_status [n_meas][S], out_sens [n_meas][n_par][S].  A kind is computed only if an output or a measure names
 * it.  A sample without an operating point has its status in sample_status, NaN rows and measure status 5; the others are served.
 * A singular Yp (a series-only network) is no failure: that (frequency, sample) has NaN in Z and dZ only.  Refused before the DC
 * solve, with the port named in ch_last_error: a port is no voltage source, appears twice, has an eliminated branch current, lacks
 * |ac| = 1 or has a multiplier other than 1; another source carries an AC magnitude; z0 is not finite and positive; a slot is a
 * port's own multiplier (CH_ERR_UNSUPPORTED); the ports' branch currents lie in separate blocks (CH_ERR_UNSUPPORTED); more than
 * 4096 coupled unknowns (CH_ERR_UNSUPPORTED); an invalid spec.  DESIGN.md 2.7k. */
int ch_net_params(ch_circuit*, const ch_dc_opts*, int32_t n_ports, const int32_t* port_devs, const double* z0, int32_t n_par, const int32_t* slot_ids,
                  const ch_sens_opts* /* NULL = defaults */, int32_t n_freq, const double* freqs_hz, double* S_out, double* Y_out, double* Z_out,
                  double* dS_out, double* dY_out, double* dZ_out, int32_t n_meas, const ch_fmeasure_spec* specs /* rows: kind * P^2 + j * P + k */,
                  double* out_value, double* out_sens, int32_t* out_status, int32_t* sample_status, ch_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* CEDARHIP_H */
