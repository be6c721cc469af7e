// Host-side print-out of recbole_amd/csrc/drop.h for tests/test_drop_header_cpu.py, which
// compares it with the numpy restatement (tests/drop_spec.py). Host compiler only:
//   c++ -std=c++17 -O1 tools/check_drop.cpp -o check_drop && ./check_drop SEED C P
// prints the key, five thresholds, then the keep bits of elements 0..4095 as drop_keep and
// as drop_keep4 see them ('1' kept).
#include <stdio.h>
#include <stdlib.h>
#include <string>

#include "../recbole_amd/csrc/drop.h"

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const uint64_t seed = strtoull(argv[1], nullptr, 0);
  const int64_t c = strtoll(argv[2], nullptr, 0);
  const double p = strtod(argv[3], nullptr);
  const uint64_t key = mirec::drop_key(seed, c);
  printf("key %llu\n", (unsigned long long)key);
  const double ps[5] = {1e-9, 0.1, 0.5, 0.9, 1.0 - ldexp(1.0, -24)};
  for (double q : ps) printf("thr %.17g %u\n", q, mirec::drop_threshold(q));
  const uint32_t thr = mirec::drop_threshold(p);
  std::string one(4096, '0'), four(4096, '0');
  for (uint64_t e = 0; e < 4096; ++e) one[e] = mirec::drop_keep(key, e, thr) ? '1' : '0';
  for (uint64_t e0 = 0; e0 < 4096; e0 += 4) {
    bool k[4];
    mirec::drop_keep4(key, e0, thr, k);
    for (int i = 0; i < 4; ++i) four[e0 + i] = k[i] ? '1' : '0';
  }
  printf("keep %s\nkeep4 %s\n", one.c_str(), four.c_str());
  return 0;
}
