// Host-only test of cedarsim.jl_amd/csrc/ch_dc_start.hpp: the cached start vector of the DC operating point and the generator
// states behind it against the loop dc_solve ran on every call before the cache, written out here with its own generator: the
// first pass' unknown-space start and three restarts' worth of draws (one of them with a sample that sits the restart out) must
// match bit for bit, for seeds 10 and 11 and S = 1 and 3.  Built with sanitizers by tests/test_host_dc_start.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ch_dc_start.hpp"

static int nbad = 0, nchecked = 0;
#define CHECK(c) do { ++nchecked; if (!(c)) { if (nbad < 40) std::printf("line %d (seed %llu, S %d): %s\n", __LINE__, (unsigned long long)g_seed, g_S, #c); ++nbad; } } while (0)
static uint64_t g_seed = 0; static int g_S = 0;

// the generator as dc_solve had it: splitmix64 + Box-Muller
struct OldRng {
  uint64_t s;
  explicit OldRng(uint64_t seed) : s(seed) {}
  uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uniform() { return ((next() >> 11) + 0.5) * (1.0 / 9007199254740992.0); }
  double normal() { double u1 = uniform(), u2 = uniform(); return std::sqrt(-2.0 * std::log(u1)) * std::cos(6.283185307179586 * u2); }
};

static bool same_bits(const double* a, const double* b, size_t n) { return n == 0 || std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
  // 29 MNA entries, 17 unknowns: several unknowns share no entry, the map is neither sorted nor contiguous
  const int n_mna = 29;
  std::vector<int> unk_mna;
  for (int u = 0; u < 17; ++u) unk_mna.push_back((u * 12 + 5) % n_mna);
  const int n_unk = (int)unk_mna.size();
  for (uint64_t seed : {10ull, 11ull}) for (int S : {1, 3}) {
    g_seed = seed; g_S = S;
    // ---- the old loop: pass r = 0 (no x0, every block active), then restarts r = 1 .. 3 ----
    std::vector<OldRng> rngs; for (int s = 0; s < S; ++s) rngs.emplace_back(seed + (uint64_t)s);
    std::vector<double> xs((size_t)S * n_unk, -1.0), xm(n_mna);
    for (int s = 0; s < S; ++s) {
      for (int i = 0; i < n_mna; ++i) xm[i] = 1e-7 * rngs[s].normal();
      for (int u = 0; u < n_unk; ++u) xs[(size_t)s * n_unk + u] = xm[unk_mna[u]];
    }
    // ---- the cache ----
    chip::DcStart st;
    CHECK(!st.matches(seed, S));
    st.fill(seed, S, n_mna, unk_mna);
    CHECK(st.matches(seed, S)); CHECK(!st.matches(seed + 1, S)); CHECK(!st.matches(seed, S + 1));
    CHECK(st.xs.size() == xs.size()); CHECK((int)st.after.size() == S);
    CHECK(st.xs.size() == xs.size() && same_bits(st.xs.data(), xs.data(), xs.size()));
    // a second fill gives the same vector and the same states (what a second circuit, or a changed and restored seed, gets)
    { chip::DcStart st2; st2.fill(seed + 5, S, n_mna, unk_mna); st2.fill(seed, S, n_mna, unk_mna);
      CHECK(same_bits(st2.xs.data(), st.xs.data(), xs.size()));
      for (int s = 0; s < S; ++s) CHECK(st2.after[s].s == st.after[s].s); }
    // ---- restarts: dc_solve copies the cached states and goes on drawing; sample 1 of a batch sits restart 2 out ----
    std::vector<chip::Rng> now = st.after;
    for (int r = 1; r <= 3; ++r) for (int s = 0; s < S; ++s) {
      if (r == 2 && s == 1) continue;
      std::vector<double> want(n_mna), got(n_mna);
      for (int i = 0; i < n_mna; ++i) want[i] = 1e-7 * rngs[s].normal();
      chip::dc_random_mna(now[s], got);
      CHECK(same_bits(want.data(), got.data(), n_mna));
      CHECK(now[s].s == rngs[s].s);
    }
    // the cache itself is untouched by the restarts of a call: the next call starts from the same states
    { std::vector<OldRng> again; for (int s = 0; s < S; ++s) again.emplace_back(seed + (uint64_t)s);
      for (int s = 0; s < S; ++s) { for (int i = 0; i < n_mna; ++i) (void)again[s].normal(); CHECK(st.after[s].s == again[s].s); } }
    // x0 given: nothing is drawn in the first pass, the restarts start from the seeds
    { std::vector<chip::Rng> fresh = chip::dc_start_rngs(seed, S);
      for (int s = 0; s < S; ++s) CHECK(fresh[s].s == seed + (uint64_t)s); }
  }
  std::printf("dc start: %d checks, %d bad\n", nchecked, nbad);
  return nbad == 0 ? 0 : 1;
}
