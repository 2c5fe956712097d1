// Host driver for csrc/krrn_so3.h (tests/test_so3_host.py): reads n row-major 3x3 f32 matrices from
// argv[1] and writes to argv[2] the n angle-axis vectors of krrn_rot_log as f64 [n][3].
#include <cstdio>
#include <vector>

#include "krrn_so3.h"

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> R;
  float buf[9];
  while (fread(buf, sizeof(float), 9, f) == 9) R.insert(R.end(), buf, buf + 9);
  fclose(f);
  const size_t n = R.size() / 9;
  std::vector<double> out(3 * n);
  for (size_t i = 0; i < n; ++i) {
    double w[3];
    krrn_rot_log(R.data() + 9 * i, w);
    for (int a = 0; a < 3; ++a) out[3 * i + a] = w[a];
  }
  f = fopen(argv[2], "wb");
  if (!f) return 4;
  const size_t wr = fwrite(out.data(), sizeof(double), out.size(), f);
  return (fclose(f) == 0 && wr == out.size()) ? 0 : 5;
}
