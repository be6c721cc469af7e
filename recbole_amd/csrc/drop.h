// The counter-based dropout draw every model kernel shares (numpy restatement:
// tests/drop_spec.py key / threshold / ln_keep; DESIGN.md "Shared device headers").
//
//   key  = mix64(mix64(seed) ^ c)            c: the site's device counter at the forward
//   thr  = min(2^32 - 1, ldexp(1 - p, 32))   an element is kept iff its 32-bit draw < thr
//   element e of a site takes half e & 1 (low half for an even e) of mix64(key ^ (e >> 1));
//   a kept element is scaled by 1 / (1 - p)
//
// Plain C++ (no HIP include): the host compiler builds it alone (tools/check_drop.cpp). A
// .hip file includes it after common.h, which brings the HIP qualifiers.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MIREC_HD __host__ __device__ __forceinline__
#else
#define MIREC_HD inline
#endif

namespace mirec {

void set_error(const char* fmt, ...);

// the splitmix64 finaliser
MIREC_HD uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the key of one draw: the seed and the counter enter separately (seed + c would give
// site s at step t + 1 the key of site s + 1 at step t: sites' seeds differ by small words)
MIREC_HD uint64_t drop_key(uint64_t seed, int64_t c) {
  return mix64(mix64(seed) ^ (uint64_t)c);
}

// keep flag of element e
MIREC_HD bool drop_keep(uint64_t key, uint64_t e, uint32_t thr) {
  const uint64_t h = mix64(key ^ (e >> 1));
  return ((e & 1) ? (uint32_t)(h >> 32) : (uint32_t)h) < thr;
}

// keep flags of the four elements e0 .. e0 + 3 (e0 a multiple of 4): two words
MIREC_HD void drop_keep4(uint64_t key, uint64_t e0, uint32_t thr, bool (&k)[4]) {
  const uint64_t h0 = mix64(key ^ (e0 >> 1)), h1 = mix64(key ^ ((e0 >> 1) + 1));
  k[0] = (uint32_t)h0 < thr;
  k[1] = (uint32_t)(h0 >> 32) < thr;
  k[2] = (uint32_t)h1 < thr;
  k[3] = (uint32_t)(h1 >> 32) < thr;
}

// keep threshold of dropout probability p (0 <= p < 1)
inline uint32_t drop_threshold(double p) {
  return (uint32_t)fmin(4294967295.0, ldexp(1.0 - p, 32));
}

// One dropout site as a kernel sees it. The forward reads the device counter c, draws from
// drop_key(seed, c) and records c in drawn[0]; the backward redraws from drawn[0] and sets
// the counter to drawn[0] + 1, the next forward's draw (one plain store each way, by the
// first thread of the grid).
struct DropSite {
  uint32_t thr;
  float scale;          // 1 / (1 - p)
  uint64_t seed;
  int64_t* counter;     // forward: read; backward: set to drawn + 1
  int64_t* drawn;       // forward writes the counter value used; backward reads it
};

inline int drop_site(float p, uint64_t seed, int64_t* counter, int64_t* drawn, DropSite* dr,
                     const char* what) {
  if (!(p > 0.f && p < 1.f) || !drawn || !counter) {
    set_error("%s: dropout %g needs 0 < p < 1, the counter and the drawn word", what, (double)p);
    return -1;
  }
  dr->thr = drop_threshold(p);
  dr->scale = 1.0f / (1.0f - p);
  dr->seed = seed;
  dr->counter = counter;
  dr->drawn = drawn;
  return 0;
}

// p == 0: a switched-off site (scale 1, no words; the kernels' no-dropout forms draw nothing)
inline int drop_site_or_off(float p, uint64_t seed, int64_t* counter, int64_t* drawn,
                            DropSite* dr, const char* what) {
  *dr = DropSite{0u, 1.f, 0ull, nullptr, nullptr};
  if (p == 0.f) return 0;
  return drop_site(p, seed, counter, drawn, dr, what);
}

}  // namespace mirec
