// Per-user register top-K lists and the history cursor shared by the full-sort scorers
// (K6 fullsort.hip, K14c neumf.hip). Both rank by (score desc, item id asc).
#pragma once
#include "common.h"

namespace mirec {

// Sorted insert into a best-first register list, branch-free (v_cndmask only;
// bitwise |/& on the predicates so clang emits no exec-mask branches).
// Scan form: strict '>' — each lane visits its items in increasing id order,
// so an equal score arriving later (higher id) correctly ranks after.
template <int KC>
__device__ __forceinline__ void topk_insert(float (&ts)[KC], int (&ti)[KC], float v, int id) {
#pragma unroll
  for (int t = KC - 1; t > 0; --t) {
    const bool up = v > ts[t - 1];
    const bool here = v > ts[t];
    const float ns = up ? ts[t - 1] : (here ? v : ts[t]);
    const int ni = up ? ti[t - 1] : (here ? id : ti[t]);
    ts[t] = ns;
    ti[t] = ni;
  }
  const bool h0 = v > ts[0];
  ts[0] = h0 ? v : ts[0];
  ti[0] = h0 ? id : ti[0];
}

// Merge form: full order (score desc, id asc) for combining two lanes' lists.
template <int KC>
__device__ __forceinline__ void topk_merge_insert(float (&ts)[KC], int (&ti)[KC], float v,
                                                  int id) {
#pragma unroll
  for (int t = KC - 1; t > 0; --t) {
    const bool up = (v > ts[t - 1]) | ((v == ts[t - 1]) & (id < ti[t - 1]));
    const bool here = (v > ts[t]) | ((v == ts[t]) & (id < ti[t]));
    const float ns = up ? ts[t - 1] : (here ? v : ts[t]);
    const int ni = up ? ti[t - 1] : (here ? id : ti[t]);
    ts[t] = ns;
    ti[t] = ni;
  }
  const bool h0 = (v > ts[0]) | ((v == ts[0]) & (id < ti[0]));
  ts[0] = h0 ? v : ts[0];
  ti[0] = h0 ? id : ti[0];
}

// History mask: a user's history is the sorted slice hist_cols[hist_ptr[q], hist_ptr[q+1]).
// First entry of cols[a, b) that is >= item (the cursor of a sweep that starts at `item`).
__device__ __forceinline__ int64_t hist_lower_bound(const int32_t* __restrict__ cols, int64_t a,
                                                    int64_t b, int64_t item) {
  while (a < b) {
    const int64_t mid = (a + b) >> 1;
    if (cols[mid] < item) a = mid + 1; else b = mid;
  }
  return a;
}

}  // namespace mirec
