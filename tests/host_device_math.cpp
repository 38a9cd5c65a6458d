// Stand-alone program of tests/test_host_device_math.py and tests/test_device_math_reference.py: the HOST instantiation of
// csrc/va_rt.hpp (the library path: what the oracle and every CPU test run) on the records of tests/device_math_cases.py.
//   host_device_math <records in> <results out>
// Records of rules that only the device has (frcp, fsqrt, flog, the DN algebra) are answered with NaN.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device_math_rules.hpp"

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  if (bytes <= 0 || bytes % (long)(dm::DM_NIN * sizeof(double)) != 0) { std::fprintf(stderr, "bad record file (%ld bytes)\n", bytes); return 2; }
  const long n = bytes / (long)(dm::DM_NIN * sizeof(double));
  std::vector<double> in((size_t)n * dm::DM_NIN), out((size_t)n * dm::DM_NOUT, NAN);
  if (std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fprintf(stderr, "short read\n"); return 2; }
  std::fclose(f);
  long done = 0;
  for (long i = 0; i < n; ++i) {
    const double* r = &in[(size_t)i * dm::DM_NIN];
    double* o = &out[(size_t)i * dm::DM_NOUT];
    switch ((int)r[0]) {
      case dm::K_SCALAR: done += dm::run_scalar_va(r, o) ? 1 : 0; break;
      case dm::K_VD1: dm::run_vd1(r, o); ++done; break;
      case dm::K_VD2: dm::run_vd2(r, o); ++done; break;
      case dm::K_INT: dm::run_int(r, o); ++done; break;
      case dm::K_SEED1: dm::run_seed1(r, o); ++done; break;
      default: break;
    }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) { std::perror(argv[2]); return 2; }
  if (std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::fprintf(stderr, "short write\n"); return 2; }
  if (std::fclose(f) != 0) { std::perror(argv[2]); return 2; }
  std::printf("device math host: %ld records, %ld evaluated\n", n, done);
  return 0;
}
