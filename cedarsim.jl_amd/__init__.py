"""cedarsim.jl_amd — MI355X-native DC/transient Newton engine behind CedarSim's problem surface.

Host-side mirror (Python) of the reference's user-facing interface for the hot path:
`Circuit` (flat device table), `dc`/`tran` (dc!/tran!, src/sweeps.jl:437-465), `CircuitSweep` and the
sweep iterators (src/sweeps.jl:150-435).  All numerics run in libcedarhip.so (HIP, gfx950) through
the C-ABI of include/cedarhip.h; there is no CPU fallback.
"""
from .circuit import (Circuit, CedarError, DC, PWL, PULSE, SIN, dc_opts, sens_opts, tran_opts, RETCODES)  # noqa: F401
from .sweeps import (Sweep, ProductSweep, TandemSweep, SerialSweep, sweepify, sweepvars, find_param_ranges, frange, shard_range)  # noqa: F401
from .netlist import parse_spice, parse_spice_file, parse_spectre_models, parse_number, NoBinException  # noqa: F401
from .api import dc, tran, ac, noise, dc_sens, acdec, ACSolution, NoiseSolution, SensSolution, CircuitSweep, Solution, gather_sharded, gather_sharded_device  # noqa: F401
from .api import ac_sens, mag_phase_sens, ACSensSolution  # noqa: F401
from .api import noise_sens, NoiseSensSolution  # noqa: F401
from .api import tran_sens, TranSensSolution  # noqa: F401
from .measure import (Measure, Event, event, when, delay, find_when, find_at, integ, avg, rms, vmin, vmax, pp, parse_measure, measure_cards,  # noqa: F401
                      resolve_measures)
from .solution import Measured, MeasureSens  # noqa: F401
from .api import ac_measure, ACMeasured  # noqa: F401
from .api import loop_gain, LoopGainSolution  # noqa: F401
from .api import net_params, NetParamsSolution  # noqa: F401
from .acmeasure import (FMeasure, FEvent, Sig, fevent, fwhen, ffind_when, ffind_at, finteg, favg, frms, fmin, fmax, fpp, db, db10, mag, phase, re, im,  # noqa: F401
                        bandwidth, unity_gain_freq, phase_margin, gain_margin, parse_ac_measure, ac_measure_cards, resolve_fmeasures, net_rows)
