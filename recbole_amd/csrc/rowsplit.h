// The row split behind every fixed-order weight-gradient sum (K16c, K18c, K19b, K20b): split
// s owns rows [s rows, (s + 1) rows) and stores one partial; mirec_linear_grad_finish_f32 adds
// the partials in split order. The split is a function of the shapes alone, so a gradient's
// bits do not depend on the device or the launch.
//
// Plain C++ (no HIP include): the host compiler builds it alone (tools/check_rowsplit.cpp).
#pragma once
#include <stdint.h>

namespace mirec {

struct RowSplit {
  int64_t rows;         // rows a split
  int splits;
};

// At most `most` splits of R > 0 rows, each a multiple of `multiple` rows and at least `least`.
inline RowSplit row_split(int64_t R, int most, int multiple, int64_t least) {
  int64_t rows = (R + most - 1) / most;
  rows = (rows + multiple - 1) / multiple * multiple;
  if (rows < least) rows = least;
  return RowSplit{rows, (int)((R + rows - 1) / rows)};
}

// a partial's stride in floats: the finish adds the partials as float4s
inline int64_t pad4(int64_t x) { return (x + 3) / 4 * 4; }

}  // namespace mirec
