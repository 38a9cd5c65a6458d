"""numpy yardstick of the BSIM4 MOSFET noise for the GPU tests: the three formula sets from operand rows (channel thermal noise of
tnoimod 0, flicker noise of fnoimod 0 and the unified model of fnoimod 1, BSIM4.5.0 manual 9.1 with lintnoi = 0), the defaults of
the noise parameters, and the assembly of an output PSD from transfers.  A plain helper module: no fixtures, no test collection.
Pinned against closed forms by test_bsim4_noise_reference.py.  Written from the formulas, independently of the engine's
ch_b4_noise.hpp: the textbook differences N0 - Nl and the logarithm of (N0 + N*)/(Nl + N*) are taken as they stand, in 50-digit
mpmath arithmetic, where their cancellation at small vds or vgsteff costs nothing."""
import mpmath
import numpy as np

KB = 1.380649e-23
Q = 1.60219e-19
OPERANDS = ("ids", "ueff", "vgsteff", "abulk", "vdseff", "vds", "rds", "esat", "litl", "leff", "weffnf", "coxe", "cdep0", "cit", "vtm", "qinv")
PARAMS = ("noia", "noib", "noic", "em", "ef", "af", "kf", "ntnoi", "tnoia", "tnoib", "rnoia", "rnoib", "fnoimod", "tnoimod")


def defaults(mtype):
    """BSIM4.5 defaults of the noise parameters for an 'n' or 'p' device."""
    n = str(mtype).lower().startswith("n")
    return dict(noia=6.25e41 if n else 6.188e40, noib=3.125e26 if n else 1.5e25, noic=8.75e9, em=4.1e7, ef=1.0, af=1.0, kf=0.0, ntnoi=1.0,
                tnoia=1.5, tnoib=3.5, rnoia=0.577, rnoib=0.5164, fnoimod=1, tnoimod=0)


def operands(row):
    """An operand row (array of 16, the engine's order) as a dict."""
    return dict(zip(OPERANDS, np.asarray(row, dtype=np.float64)))


def thermal(op, par, T):
    """Channel thermal noise, tnoimod 0 [A^2/Hz]: 4kT ntnoi ueff|qinv| / (leff^2 + ueff|qinv| rds)."""
    uq = op["ueff"] * abs(op["qinv"])
    return 4.0 * KB * T * par["ntnoi"] * uq / (op["leff"] ** 2 + uq * op["rds"])


def flicker_simple(op, par):
    """fnoimod 0 at 1 Hz [A^2/Hz]: kf |ids|^af / (coxe leff^2)."""
    return par["kf"] * abs(op["ids"]) ** par["af"] / (op["coxe"] * op["leff"] ** 2) if par["kf"] != 0.0 else 0.0


def unified_parts(op, par, T):
    """(S_inv, S_wi) of the unified model at 1 Hz, as mpmath numbers of 50 digits."""
    with mpmath.workdps(50):
        L = mpmath.mpf
        ids, ueff, vg, ab, vde, vtm = (L(abs(float(op["ids"]))), L(float(op["ueff"])), L(float(op["vgsteff"])), L(float(op["abulk"])), L(float(op["vdseff"])), L(float(op["vtm"])))
        coxe, leff, wn, litl, kT, q = L(float(op["coxe"])), L(float(op["leff"])), L(float(op["weffnf"])), L(float(op["litl"])), L(KB) * L(float(T)), L(Q)
        a, b, c = L(float(par["noia"])), L(float(par["noib"])), L(float(par["noic"]))
        N0 = coxe * vg / q
        Nl = coxe * vg * (1 - ab * vde / (vg + 2 * vtm)) / q
        Ns = vtm * (coxe + L(float(op["cdep0"])) + L(float(op["cit"]))) / q
        dl = litl * mpmath.log(((L(float(op["vds"])) - vde) / litl + L(float(par["em"]))) / L(float(op["esat"])))
        dl = dl if dl > 0 else L(0)
        s_inv = kT * q * q * ueff * ids / (coxe * leff ** 2 * ab * L(1e10)) * (a * mpmath.log((N0 + Ns) / (Nl + Ns)) + b * (N0 - Nl) + L(0.5) * c * (N0 ** 2 - Nl ** 2)) \
            + kT * ids ** 2 * dl / (wn * leff ** 2 * L(1e10)) * (a + b * Nl + c * Nl ** 2) / (Nl + Ns) ** 2
        s_wi = a * kT * ids ** 2 / (wn * leff * Ns ** 2 * L(1e10))
        return s_inv, s_wi


def flicker_unified(op, par, T):
    """fnoimod 1 at 1 Hz [A^2/Hz]: the harmonic mean of S_inv and S_wi."""
    if op["ids"] == 0.0:
        return 0.0
    s_inv, s_wi = unified_parts(op, par, T)
    with mpmath.workdps(50):
        return float(s_inv * s_wi / (s_inv + s_wi)) if s_inv + s_wi > 0 else 0.0


def records(op, par, T, m=1.0):
    """[(pwr, exponent)] of one MOSFET: thermal, flicker; times the multiplier."""
    fl = flicker_simple(op, par) if int(par["fnoimod"]) == 0 else flicker_unified(op, par, T)
    return [(m * thermal(op, par, T), 0.0), (m * fl, par["ef"])]


def psd_from_transfers(H, table, f):
    """Output PSD over the frequencies f [Hz]: sum_k |H_k(f)|^2 pwr_k / f^ex_k, H[k] the transfer from a unit current through
    source k to the output (array over f), table[k] = (pwr, exponent)."""
    f = np.asarray(f, dtype=np.float64)
    out = np.zeros(len(f))
    for Hk, (pwr, ex) in zip(H, table):
        out += np.abs(np.asarray(Hk)) ** 2 * (pwr if ex == 0.0 else pwr / f ** ex)
    return out
