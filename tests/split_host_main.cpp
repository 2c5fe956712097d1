// Host driver for csrc/krrn_split.h (tests/test_split_host.py): reads n f32 values (n a multiple of
// 4) from argv[1] and writes to argv[2] the bf16 bit patterns h[n], m[n], l[n] of krrn_split3, then
// h[n], m[n], l[n] of krrn_split3_pair, as uint16.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "krrn_split.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

static void put(std::vector<uint16_t>& d, size_t i, unsigned w) {
  d[i] = (uint16_t)(w & 0xFFFFu);
  d[i + 1] = (uint16_t)(w >> 16);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> x;
  float buf[4];
  while (fread(buf, sizeof(float), 4, f) == 4) x.insert(x.end(), buf, buf + 4);
  fclose(f);
  const size_t n = x.size();
  std::vector<uint16_t> out(6 * n);
  for (size_t i = 0; i < n; i += 4) {
    const KrrnSplit3 s = krrn_split3(f32x4{x[i], x[i + 1], x[i + 2], x[i + 3]});
    put(out, i, s.h0), put(out, i + 2, s.h1);
    put(out, n + i, s.m0), put(out, n + i + 2, s.m1);
    put(out, 2 * n + i, s.l0), put(out, 2 * n + i + 2, s.l1);
  }
  for (size_t i = 0; i < n; i += 2) {
    const KrrnSplit3Pair s = krrn_split3_pair(f32x2{x[i], x[i + 1]});
    put(out, 3 * n + i, s.h), put(out, 4 * n + i, s.m), put(out, 5 * n + i, s.l);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 4;
  const size_t w = fwrite(out.data(), sizeof(uint16_t), out.size(), f);
  return (fclose(f) == 0 && w == out.size()) ? 0 : 5;
}
