// Replays the sparse plan of ch_sparse_host.hpp on a matrix read from a file (tests/golden/mna_jacobian_*.txt) the way the GPU kernels
// do — static pivot sequence, no search — and checks the residual of a solve.  Regression test for the zero pivots that ideal and
// controlled sources produce in MNA matrices after a few eliminations (scripts/extended_fuzz.py, seed 20095).
#include <cstdio>
#include <cmath>
#include <random>
#include <vector>
#include "../cedarsim.jl_amd/csrc/ch_sparse_host.hpp"
using namespace chip;
int main(int argc, char** argv) {
  int bad = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "r"); int n;
    if (!f || fscanf(f, "%d", &n) != 1) { printf("cannot read %s\n", argv[a]); return 2; }
    std::vector<int> rp(1, 0), ci; std::vector<double> av;
    for (int i = 0; i < n; ++i) { int m; if (fscanf(f, "%d", &m) != 1) return 2; for (int q = 0; q < m; ++q) { int j; double v; if (fscanf(f, "%d %lf", &j, &v) != 2) return 2; ci.push_back(j); av.push_back(v); } rp.push_back((int)ci.size()); }
    fclose(f);
    SparsePlan P;
    if (sparse_analyse(n, rp, ci, av, P) != CH_OK) { printf("%s: analysis failed\n", argv[a]); ++bad; continue; }
    std::vector<double> b(n);
    std::mt19937 rng(1); for (int i = 0; i < n; ++i) b[i] = ((int)(rng() % 200) - 100) / 10.0;
    const SparseReplay rep = sparse_replay(P, av, b);
    const std::vector<double>& dx = rep.x; const double minpiv = rep.min_pivot;
    double rmax = 0, bmax = 0; bool finite = true;
    for (int i = 0; i < n; ++i) { double s = -b[i]; for (int p = rp[i]; p < rp[i + 1]; ++p) s += av[p] * dx[ci[p]]; if (!std::isfinite(s)) finite = false; rmax = std::max(rmax, std::fabs(s)); bmax = std::max(bmax, std::fabs(b[i])); }
    printf("%s: n %d nnz(L+U) %d min |pivot| %.3e residual %.3e of %.3e\n", argv[a], n, P.nnz_lu, minpiv, rmax, bmax);
    if (!finite || !(minpiv > 0.0) || !(rmax <= 1e-8 * bmax)) ++bad;
  }
  printf("%d bad\n", bad);
  return bad ? 1 : 0;
}
