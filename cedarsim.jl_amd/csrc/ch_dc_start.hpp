// ch_dc_start.hpp — the random start of the DC operating point, HIP-free: the generator (u0 = 1e-7*randn, dcop.jl:60), the rule
// "MNA start -> unknown-space state", and the per-circuit cache of the first pass' start vector.  The numbers of the first pass
// are a pure function of (seed, S, n_mna) and of the circuit's unknown map, so a circuit draws them once: DcStart keeps the
// unknown-space start and every sample's generator state BEHIND that fill, from which the restarts go on drawing exactly the
// numbers they drew when every call started from the seed.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace chip {

// ---- RNG: splitmix64 + Box-Muller, as specified for the DC initial guess u0 = 1e-7*randn (dcop.jl:60)
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uniform() { return ((next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal() { double u1 = uniform(), u2 = uniform(); return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2); }
};

// sample s of a batch draws from its own generator
inline std::vector<Rng> dc_start_rngs(uint64_t seed, int S) {
  std::vector<Rng> r; r.reserve((size_t)S);
  for (int s = 0; s < S; ++s) r.emplace_back(seed + (uint64_t)s);
  return r;
}
// one sample's random MNA start: n_mna draws, in MNA order
inline void dc_random_mna(Rng& rng, std::vector<double>& xm) { for (double& v : xm) v = 1e-7 * rng.normal(); }
// MNA start -> the unknowns of one sample: unknown u takes the value of its representative MNA entry
inline void dc_mna_to_unknowns(const double* xm, const std::vector<int>& unk_mna, double* xs) {
  for (size_t u = 0; u < unk_mna.size(); ++u) xs[u] = xm[unk_mna[u]];
}

// The first pass of a DC solve that has no x0 (every block active): [S][n_unk] start and the generators behind it.
struct DcStart {
  bool valid = false; uint64_t seed = 0; int S = 0;
  std::vector<double> xs;      // unknown-space start, as the first pass writes it into the ring slot
  std::vector<Rng> after;      // every sample's generator after its n_mna draws: where the restarts continue
  bool matches(uint64_t sd, int s) const { return valid && seed == sd && S == s; }
  void fill(uint64_t sd, int s, int n_mna, const std::vector<int>& unk_mna) {
    seed = sd; S = s; valid = true;
    after = dc_start_rngs(sd, s);
    xs.assign((size_t)s * unk_mna.size(), 0.0);
    std::vector<double> xm((size_t)n_mna);
    for (int q = 0; q < s; ++q) { dc_random_mna(after[q], xm); dc_mna_to_unknowns(xm.data(), unk_mna, xs.data() + (size_t)q * unk_mna.size()); }
  }
};

}  // namespace chip
