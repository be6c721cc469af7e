// Decoupled look-back words: how the workgroups of one launch learn the counts of the
// workgroups before them (segsort.hip's onesweep passes and segment scan, segreduce.hip's
// merge). The contract of every user:
//   * the words (and the launch's ticket) are zero before a launch and are left zero: the
//     last block of the launch (os_cleanup) zeroes what the launch used;
//   * a block publishes its own count (kOsFlagA | count) BEFORE it sums its
//     predecessors', so no wait chains through predecessors and every wait ends;
//   * a word carries only its own count — no data is published through it — so relaxed
//     agent-scope loads and stores suffice, and the loads of many predecessors can be in
//     flight together (an acquire load waits for itself).
#pragma once
#include "common.h"

namespace mirec {

constexpr uint32_t kOsFlagA = 1u << 30, kOsVal = (1u << 30) - 1;

__device__ __forceinline__ uint32_t os_load(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void os_store(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// sum of the counts of tiles h, h + H, h + 2H, ... < tile in column `words` (stride per
// tile): 16 loads in flight per batch, a word not yet published is re-read
__device__ __forceinline__ uint32_t os_sum_before(const uint32_t* words, int64_t tile,
                                                  int64_t stride, int h, int H) {
  uint32_t s = 0;
  for (int64_t t0 = h; t0 < tile; t0 += 16 * (int64_t)H) {
    uint32_t w[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int64_t t = t0 + j * (int64_t)H;
      w[j] = t < tile ? os_load(words + t * stride) : kOsFlagA;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int64_t t = t0 + j * (int64_t)H;
      while ((w[j] >> 30) == 0) {
        __builtin_amdgcn_s_sleep(1);
        w[j] = os_load(words + t * stride);
      }
      s += t < tile ? (w[j] & kOsVal) : 0u;
    }
  }
  return s;
}

// the last of the launch's blocks (ticket) zeroes `words` [0, n_words)
__device__ __forceinline__ void os_cleanup(uint32_t* ticket, uint32_t* words, int64_t n_words,
                                           int* flag_lds) {
  __syncthreads();
  if (threadIdx.x == 0)
    *flag_lds = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                gridDim.x - 1;
  __syncthreads();
  if (*flag_lds) {
    for (int64_t q = threadIdx.x; q < n_words; q += blockDim.x) words[q] = 0u;
    if (threadIdx.x == 0) *ticket = 0u;
  }
}

}  // namespace mirec
