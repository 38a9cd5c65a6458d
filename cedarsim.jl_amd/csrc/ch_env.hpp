// ch_env.hpp — every environment switch the engine reads, in one table (HIP-free).
//
// None of them is part of the supported interface (that is include/cedarhip.h); they exist for the tests' A/B runs, for test
// hooks that force a rare path, and for diagnostics.  The environment is read AT CALL TIME: the tests flip switches between
// calls in one process, so nothing here is cached (the two per-circuit reads, HOST_PROFILE and TIME_EVERY, happen when a
// circuit is constructed).  A switch is named by its enumerator, so a name that is not in the table does not compile.
#pragma once

#include <cstdlib>

namespace chip {

enum class EnvKind { TEST_HOOK, DIAGNOSTIC, AB_SWITCH };   // forces a rare path | prints or measures, results unchanged | selects another implemented path

struct EnvSwitch { const char* name; EnvKind kind; const char* what; };

enum class Env {
  STEPPER, LOCKSTEP, NO_TEAR, TORN_DC_SPARSE, PERSIST_NOPAIR, FORCE_SPARSE, SPARSE_ONE_WG, SPARSE_NO_SUBTREE, BP_RESTART_ALL,
  VA_NOSPLIT, VA_NO_LDS, DEVICE_REDUCE, PERSIST_MAXROWS, SPIN_TICKS, TIME_EVERY, HOST_PROFILE, DEBUG_BLOB, DEBUG_TORN,
  DEBUG_STEPPER, DEBUG_AC, PAIR_DBG, MEASURE_SPLIT, MEASURE_CAP, COUNT
};

// same order as the enumerators
constexpr EnvSwitch ENV_SWITCHES[] = {
  {"CEDARHIP_STEPPER", EnvKind::AB_SWITCH, "host|device: step controller when ch_tran_opts.stepper is AUTO (the option itself wins otherwise)"},
  {"CEDARHIP_LOCKSTEP", EnvKind::AB_SWITCH, "independent blocks / samples on a saveat grid keep ONE step sequence (= step_control CH_STEPS_SHARED)"},
  {"CEDARHIP_NO_TEAR", EnvKind::AB_SWITCH, "a coupled array that could be torn at its rails stays on the sparse path"},
  {"CEDARHIP_TORN_DC_SPARSE", EnvKind::AB_SWITCH, "only the operating point of a torn array goes to the sparse path"},
  {"CEDARHIP_PERSIST_NOPAIR", EnvKind::AB_SWITCH, "device stepper without the function split across wave pairs"},
  {"CEDARHIP_FORCE_SPARSE", EnvKind::AB_SWITCH, "every circuit on path 2 (sparse level-scheduled LU)"},
  {"CEDARHIP_SPARSE_ONE_WG", EnvKind::AB_SWITCH, "sparse path: the one-workgroup LU instead of the multi-workgroup forms"},
  {"CEDARHIP_SPARSE_NO_SUBTREE", EnvKind::AB_SWITCH, "sparse path: the level-synchronous kernels instead of the subtree form"},
  {"CEDARHIP_BP_RESTART_ALL", EnvKind::AB_SWITCH, "restart at order 1 behind EVERY break point (the oracle reads it too)"},
  {"CEDARHIP_VA_NOSPLIT", EnvKind::AB_SWITCH, "compiled Verilog-A devices evaluated whole by one lane group (no resistive / charge halves)"},
  {"CEDARHIP_VA_NO_LDS", EnvKind::AB_SWITCH, "device stepper: parameter and constant blocks of compiled devices are not staged in LDS"},
  {"CEDARHIP_DEVICE_REDUCE", EnvKind::AB_SWITCH, "block records reduced by reduce_blocks_kernel at any batch size"},
  {"CEDARHIP_PERSIST_MAXROWS", EnvKind::TEST_HOOK, "row buffer of the device stepper (forces the drain-and-resume path)"},
  {"CEDARHIP_SPIN_TICKS", EnvKind::TEST_HOOK, "bound of every grid-wide wait in 10 ns ticks (1: every wait gives up at once: exercises the fallback)"},
  {"CEDARHIP_TIME_EVERY", EnvKind::DIAGNOSTIC, "kernel timing events on every n-th launch of the host stepper (default 8); per circuit"},
  {"CEDARHIP_HOST_PROFILE", EnvKind::DIAGNOSTIC, "host-side time split of every transient on stderr; per circuit"},
  {"CEDARHIP_DEBUG_BLOB", EnvKind::DIAGNOSTIC, "sizes of the per-class gather lists on stderr"},
  {"CEDARHIP_DEBUG_TORN", EnvKind::DIAGNOSTIC, "timeline of the torn form's operating point on stderr"},
  {"CEDARHIP_DEBUG_STEPPER", EnvKind::DIAGNOSTIC, "why the host stepper was taken; LDS budget of the device stepper"},
  {"CEDARHIP_DEBUG_AC", EnvKind::DIAGNOSTIC, "the linearisation an AC analysis starts from (one small block)"},
  {"CEDARHIP_PAIR_DBG", EnvKind::DIAGNOSTIC, "PersistArgs::pair_dbg: diagnostic variants of the wave-pair evaluation"},
  {"CEDARHIP_MEASURE_SPLIT", EnvKind::AB_SWITCH, "lanes|time: kernel form of the waveform and the frequency-domain measurements (anything else, or unset: a lane per sample from 64 samples up, else a wavefront per sample)"},
  {"CEDARHIP_MEASURE_CAP", EnvKind::TEST_HOOK, "doubles of rows one launch of the waveform or frequency-domain measurements may hold instead of DENSE_WORK_CAP (forces the sample-chunk path)"},
};
static_assert(sizeof(ENV_SWITCHES) / sizeof(ENV_SWITCHES[0]) == (size_t)Env::COUNT, "ENV_SWITCHES lists every Env enumerator, in order");

inline const char* env_get(Env e) { return std::getenv(ENV_SWITCHES[(int)e].name); }
inline bool env_on(Env e) { return env_get(e) != nullptr; }
inline long env_long(Env e, long dflt) { const char* v = env_get(e); return v ? std::atol(v) : dflt; }

}  // namespace chip
