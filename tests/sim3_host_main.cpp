// Host driver for csrc/krrn_umeyama.h (tests/test_sim3_host.py): reads n records of 16 f64
// (mS[3], mT[3], Cov[9] row-major, varP) from argv[1] and writes to argv[2] the n results of
// umeyama_solve as 13 f64 each (s, R[9] row-major, t[3]).
#include <cstdio>
#include <vector>

#include "krrn_umeyama.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<double> in;
  double buf[16];
  while (fread(buf, sizeof(double), 16, f) == 16) in.insert(in.end(), buf, buf + 16);
  fclose(f);
  const size_t n = in.size() / 16;
  std::vector<double> out(13 * n);
  for (size_t i = 0; i < n; ++i) {
    const double* r = in.data() + 16 * i;
    double mS[3], mT[3], Cov[9];
    for (int a = 0; a < 3; ++a) {
      mS[a] = r[a];
      mT[a] = r[3 + a];
    }
    for (int a = 0; a < 9; ++a) Cov[a] = r[6 + a];
    Sim sim;
    umeyama_solve(mS, mT, Cov, r[15], sim);
    out[13 * i] = sim.s;
    for (int a = 0; a < 9; ++a) out[13 * i + 1 + a] = sim.R[a];
    for (int a = 0; a < 3; ++a) out[13 * i + 10 + a] = sim.t[a];
  }
  f = fopen(argv[2], "wb");
  if (!f) return 4;
  const size_t wr = fwrite(out.data(), sizeof(double), out.size(), f);
  return (fclose(f) == 0 && wr == out.size()) ? 0 : 5;
}
