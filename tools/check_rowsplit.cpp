// Host-side print-out of recbole_amd/csrc/rowsplit.h for tests/test_rowsplit_cpu.py, which
// compares it with the four kernels' split rules written out one by one. Host compiler only:
//   c++ -std=c++17 -O1 tools/check_rowsplit.cpp -o check_rowsplit && ./check_rowsplit < tuples
// reads "R most multiple least" lines from stdin and prints "rows splits" for each.
#include <inttypes.h>
#include <stdio.h>

#include "../recbole_amd/csrc/rowsplit.h"

int main() {
  int64_t R, least;
  int most, multiple;
  while (scanf("%" SCNd64 " %d %d %" SCNd64, &R, &most, &multiple, &least) == 4) {
    const mirec::RowSplit sp = mirec::row_split(R, most, multiple, least);
    printf("%" PRId64 " %d\n", sp.rows, sp.splits);
  }
  return 0;
}
