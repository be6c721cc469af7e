// K2 — deterministic grouping of gradient contributions by table row.
//
// torch's nn.Embedding(sparse=False) backward (bpr.py:40-41) zero-fills a dense
// [n_rows, d] gradient and index_adds every looked-up row into it.  Here the
// contributions are grouped instead: a stable LSD radix sort of (row id,
// contribution index) gives, per distinct row, the ordered list of its
// contributions, which K5 (adam.hip) or the dense scatter (segreduce.hip) sums in
// that fixed order — bitwise reproducible, no float atomics.
//
// The sort runs in ONE workgroup (512 lanes): n is a training batch's
// contribution count (C2: 512 user keys, 2,560 item keys), far too small to
// fill the chip, and the sort depends only on ids, so the trainer runs it
// ahead of the model step on a side stream.  Up to kLdsMax keys the whole
// sort lives in LDS (stable kDigitBits-bit digit passes, packed per-thread digit
// counts, one block scan per pass). Larger batches: one large batch takes a
// device-wide LSD radix sort (upsweep histograms, scan, stable downsweep), several
// take one workgroup each over global ping-pong buffers (1-bit stable splits).
#include "common.h"
#include "ahead.h"
#include "lookback.h"

namespace mirec {

#ifndef MIREC_SORT_THREADS
#define MIREC_SORT_THREADS 512
#endif
// 512 lanes: each 4-bit pass pays a fixed cross-wave cost (wave scan, per-wave totals,
// two barriers) that grows with the wave count — one C2 batch (512 user keys / 2,560 item
// keys) sorts in 14.7 / 20.3 us with 8 waves against 27.1 / 29.1 us with 16
// (tools/probe_segsort.py, variants by tools/build_variant.sh -DMIREC_SORT_THREADS=N).
constexpr int kSortThreads = MIREC_SORT_THREADS;
#ifndef MIREC_SORT_DIGIT_BITS
#define MIREC_SORT_DIGIT_BITS 4
#endif
constexpr int kDigitBits = MIREC_SORT_DIGIT_BITS;      // radix digit width of the LDS sort
constexpr int kDigitWords = (1 << kDigitBits) / 4;     // four 16-bit counters per 64-bit word
constexpr int kLdsMax = 8192;
constexpr int kIpt = kLdsMax / kSortThreads;  // items per thread in the LDS path
// knobs of the probing builds (tools/build_variant.sh): digits of 2..6 bits (kDigitWords
// packed words of four 16-bit counters each), whole waves dividing the LDS capacity
static_assert(kDigitBits >= 2 && kDigitBits <= 6, "MIREC_SORT_DIGIT_BITS must be in [2, 6]");
static_assert(kSortThreads % 64 == 0 && kSortThreads <= 1024 && kLdsMax % kSortThreads == 0,
              "MIREC_SORT_THREADS: a multiple of 64, at most 1024, dividing kLdsMax");

__host__ __device__ __forceinline__ int nbits_for(int64_t key_space) {
  int b = 0;
  while (b < 31 && ((int64_t)1 << b) < key_space) ++b;
  return b;
}

// uniq/seg from sorted keys held in `skey` (LDS or global), blocked arrangement
template <typename KeyPtr>
__device__ void emit_segments(KeyPtr skey, int n, int32_t* __restrict__ uniq,
                              int32_t* __restrict__ seg, int32_t* __restrict__ n_uniq,
                              int* scan_lds) {
  int base_u = 0;
  for (int c0 = 0; c0 < n; c0 += kSortThreads) {
    const int i = c0 + threadIdx.x;
    int f = 0;
    int32_t kv = 0;
    if (i < n) {
      kv = skey[i];
      f = (i == 0 || skey[i - 1] != kv) ? 1 : 0;
    }
    int tot;
    const int ex = block_exclusive_scan(f, scan_lds, &tot);
    if (f) {
      uniq[base_u + ex] = kv;
      seg[base_u + ex] = i;
    }
    base_u += tot;
  }
  if (threadIdx.x == 0) {
    seg[base_u] = n;
    n_uniq[0] = base_u;
  }
}

// One workgroup per batch: batch b sorts keys[b*batch_n, min((b+1)*batch_n, n_total))
// and writes perm/uniq at b*batch_n, seg at b*(batch_n+1), n_uniq[b].
struct SortLds {
  int32_t kA[kLdsMax], vA[kLdsMax], kB[kLdsMax], vB[kLdsMax];
  int scan[kSortThreads / 64 + 1];
  uint64_t wtot[kSortThreads / 64][kDigitWords];  // per-wave packed digit counts
};
// the two-job kernel (segsort_lds2_kernel) holds one SortLds; gfx950 has 160 KiB per CU
static_assert(sizeof(SortLds) <= 160 * 1024, "SortLds exceeds the gfx950 LDS");

__device__ __forceinline__ void segsort_lds_batch(
    const int64_t* __restrict__ keys_all, int64_t n_total, int batch_n, int nbits,
    int32_t* __restrict__ perm_all, int32_t* __restrict__ uniq_all,
    int32_t* __restrict__ seg_all, int32_t* __restrict__ n_uniq_all, int64_t b, SortLds& L) {
  int32_t* kA = L.kA;
  int32_t* vA = L.vA;
  int32_t* kB = L.kB;
  int32_t* vB = L.vB;
  int* scan_lds = L.scan;
  const int n = (int)min((int64_t)batch_n, n_total - b * batch_n);
  const int64_t* __restrict__ keys = keys_all + b * batch_n;
  int32_t* __restrict__ perm = perm_all + b * batch_n;
  int32_t* __restrict__ uniq = uniq_all + b * batch_n;
  int32_t* __restrict__ seg = seg_all + b * (batch_n + 1);
  int32_t* __restrict__ n_uniq = n_uniq_all + b;
  for (int i = threadIdx.x; i < n; i += kSortThreads) {
    kA[i] = (int32_t)keys[i];
    vA[i] = i;
  }
  __syncthreads();
  int32_t *ks = kA, *vs = vA, *kd = kB, *vd = vB;
  const int ipt = (n + kSortThreads - 1) / kSortThreads;
  const int lo = threadIdx.x * ipt;
  const int hi = min(n, lo + ipt);
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  constexpr int nw = kSortThreads / 64;  // every launch of these kernels: kSortThreads lanes
  // Stable LSD passes of kDigitBits-bit digits (a blocked arrangement: thread t owns
  // positions [lo, hi)). Per-digit counts travel packed, four 16-bit fields per
  // 64-bit word (n <= 8192 < 2^16: no carries), so one wave scan of kDigitWords words
  // and one barrier give every thread its per-digit exclusive prefix; the
  // destination of an item is (items of smaller digits) + (items of its digit
  // before it) — the same permutation as 1-bit splits, in 1/kDigitBits of the
  // passes.
  for (int shift = 0; shift < nbits; shift += kDigitBits) {
    constexpr int kMask = (1 << kDigitBits) - 1;
    uint64_t c[kDigitWords];
#pragma unroll
    for (int w = 0; w < kDigitWords; ++w) c[w] = 0ull;
    for (int i = lo; i < hi; ++i) {
      const int d = (ks[i] >> shift) & kMask;
#pragma unroll
      for (int w = 0; w < kDigitWords; ++w) c[w] += (d >> 2) == w ? 1ull << (16 * (d & 3)) : 0ull;
    }
    uint64_t inc[kDigitWords];
#pragma unroll
    for (int w = 0; w < kDigitWords; ++w) inc[w] = c[w];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
      for (int w = 0; w < kDigitWords; ++w) {
        const uint64_t y = __shfl_up(inc[w], off, 64);
        if (lane >= off) inc[w] += y;
      }
    }
    if (lane == 63) {
#pragma unroll
      for (int w = 0; w < kDigitWords; ++w) L.wtot[wid][w] = inc[w];
    }
    __syncthreads();
    uint64_t ex[kDigitWords], tot[kDigitWords];
#pragma unroll
    for (int w = 0; w < kDigitWords; ++w) { ex[w] = inc[w] - c[w]; tot[w] = 0ull; }
#pragma unroll
    for (int v = 0; v < nw; ++v) {
#pragma unroll
      for (int w = 0; w < kDigitWords; ++w) {
        const uint64_t x = L.wtot[v][w];
        ex[w] += v < wid ? x : 0ull;
        tot[w] += x;
      }
    }
    auto fsum = [](uint64_t x) {     // sum of the four 16-bit fields
      return (int)((x & 0xffff) + ((x >> 16) & 0xffff) + ((x >> 32) & 0xffff) + (x >> 48));
    };
    for (int i = lo; i < hi; ++i) {
      const int32_t kv = ks[i];
      const int d = (kv >> shift) & kMask;
      const int w = d >> 2, f = 16 * (d & 3);
      int base = 0;
      uint64_t e = 0ull;
#pragma unroll
      for (int q = 0; q < kDigitWords; ++q) {
        base += q < w ? fsum(tot[q]) : 0;
        if (q == w) {
          base += fsum(tot[q] & ((1ull << f) - 1ull));
          e = ex[q];
          ex[q] += 1ull << f;
        }
      }
      const int dst = base + (int)((e >> f) & 0xffff);
      kd[dst] = kv;
      vd[dst] = vs[i];
    }
    __syncthreads();
    int32_t* t;
    t = ks; ks = kd; kd = t;
    t = vs; vs = vd; vd = t;
  }
  for (int i = threadIdx.x; i < n; i += kSortThreads) perm[i] = vs[i];
  emit_segments(ks, n, uniq, seg, n_uniq, scan_lds);
}

__global__ __launch_bounds__(kSortThreads) void segsort_lds_kernel(
    const int64_t* __restrict__ keys_all, int64_t n_total, int batch_n, int nbits,
    int32_t* __restrict__ perm_all, int32_t* __restrict__ uniq_all,
    int32_t* __restrict__ seg_all, int32_t* __restrict__ n_uniq_all) {
  __shared__ SortLds L;
  segsort_lds_batch(keys_all, n_total, batch_n, nbits, perm_all, uniq_all, seg_all, n_uniq_all,
                    blockIdx.x, L);
}

// Per-block stable sort for blocks of <= kR8Max keys whatever the key space or the
// duplicates (DeepFM's field blocks: 2,048 ids of up to 10 M rows, Zipf heads and
// small-vocabulary fields alike): LSD passes of 8-bit digits over (key - the block's
// minimum) — ceil(bits of the block's key span / 8) passes instead of 4-bit passes over
// the table's id width. Wave w owns a contiguous run of 64-key chunks; in each chunk the
// 8 digit-bit ballots intersect to every lane's set of same-digit lanes, so a key's rank
// is (its digit's count in the wave's earlier chunks, an LDS counter [digit][wave] the
// digit's leader lane advances) + (same-digit lanes below it). One block scan of the
// 256 x 8 counters (digit-major) gives every (digit, wave) its output offset — stable,
// no atomics. Same perm / uniq / seg / n_uniq as segsort_lds_batch.
#ifndef MIREC_R8_THREADS
#define MIREC_R8_THREADS 512
#endif
// (1,024 lanes — half the chunks per wave — measured the same: C4 grouping 24.6 vs 25.3 us
// by events, 11.81 vs 11.82 M samples/s)
constexpr int kR8Threads = MIREC_R8_THREADS;
constexpr int kR8Waves = kR8Threads / 64;
constexpr int kR8Max = 4096;
constexpr int kChainMaxBlocks = 256;       // chained look-back: at most 4 loads per lane
struct R8Lds {
  uint32_t k[2][kR8Max];                   // the block's keys (int32 bit patterns)
  uint16_t v[2][kR8Max];                   // their positions in the block
  uint16_t rank[kR8Max];                   // a key's rank among its digit in its wave
  int hist[256 * kR8Waves];                // [digit][wave] counts, then their offsets
  int scan[kR8Waves + 1];
  int32_t kmin, kmax, base, last;
};

// The ballot ranking of one 64-key chunk by 8-bit digit within its wave (this kernel and
// the onesweep passes, os_pass_kernel): the 8 digit-bit ballots intersect to the lane's
// set of same-digit lanes m (lt: the mask of the lanes below this one). cnt[digit][wid]
// of the [256][W waves] counters is the digit's count in the wave's earlier chunks,
// which the digit's leader lane advances between two wave barriers; rank[i] (key i, if
// valid) = that count + the same-digit lanes below. A fix here reaches both sorts.
template <int W>
__device__ __forceinline__ void rank_chunk8(uint32_t dd, bool valid, uint64_t lt, int* cnt,
                                            int wid, uint16_t* rank, int i) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int bb = 0; bb < 8; ++bb) {             // same-digit lanes: AND of xnor(ballot, bit)
    const int32_t sb = __builtin_amdgcn_sbfe((int32_t)dd, bb, 1);
    const uint64_t bl = __ballot(sb != 0);
    m &= ~(bl ^ (uint64_t)(int64_t)sb);
  }
  const int r = __popcll(m & lt);
  int* h = &cnt[(int)dd * W + wid];
  const int before = valid ? *h : 0;
  __builtin_amdgcn_wave_barrier();
  if (valid && r == 0) *h = before + __popcll(m);
  __builtin_amdgcn_wave_barrier();
  if (valid) rank[i] = (uint16_t)(before + r);
}

// Exclusive scan, digit-major, of the 256 x W counters of a block of T lanes (in place):
// every (digit, wave) gets the offset of its keys in the block's output.
template <int W, int T>
__device__ __forceinline__ void scan_digit_counters(int* cnt, int* scan_lds) {
  constexpr int per = 256 * W / T;
  const int tid = threadIdx.x;
  int c[per], sum = 0;
#pragma unroll
  for (int q = 0; q < per; ++q) {
    c[q] = cnt[tid * per + q];
    sum += c[q];
  }
  int tot;
  int run = block_exclusive_scan(sum, scan_lds, &tot);
#pragma unroll
  for (int q = 0; q < per; ++q) {
    cnt[tid * per + q] = run;
    run += c[q];
  }
}

#ifdef MIREC_R8_PROBE
__device__ uint64_t g_r8_probe[16];
#define R8T(k) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_r8_probe[k] = wall_clock64(); } while (0)
#define R8C(k) do { if (threadIdx.x == 0 && blockIdx.x == 0) g_r8_probe[k] = clock64(); } while (0)
extern "C" int mirec_r8_probe_read(uint64_t* host) {
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_r8_probe), sizeof(g_r8_probe)) == hipSuccess ? 0 : -1;
}
#else
#define R8T(k) do {} while (0)
#define R8C(k) do {} while (0)
#endif
// status == nullptr: block b writes its own perm / uniq / seg / n_uniq at b's offsets in
// the outputs (block-local positions; blocks_concat_kernel joins them). status != nullptr
// (chained, one launch): block b publishes its unique count in status[b] (count + 1,
// release), sums the counts of blocks < b (acquire; every one of them was dispatched
// before b and publishes without waiting, so the wait ends) and writes straight into the
// concatenated outputs; the block that takes the last ticket in status[nblocks] zeroes
// status again for the next launch.
// Keys given as fields (DeepFM: block b = field b's column + the field's table offset):
// the kernel forms them itself and writes them out for the forward's gathers.
constexpr int kSortFields = 64;
struct SortFields {
  const int64_t* col[kSortFields];
  int64_t off[kSortFields];
  int64_t* keys_out;
};

__global__ __launch_bounds__(kR8Threads) void segsort_radix8_kernel(
    const int64_t* __restrict__ keys_all, int64_t n_total, int batch_n,
    int32_t* __restrict__ perm_all, int32_t* __restrict__ uniq_all,
    int32_t* __restrict__ seg_all, int32_t* __restrict__ n_uniq_all,
    int32_t* __restrict__ status, int32_t* __restrict__ pu_all, const SortFields SF) {
  __shared__ R8Lds L;
  R8T(0);
  R8C(12);
  const int64_t b = blockIdx.x;
  const int n = (int)min((int64_t)batch_n, n_total - b * batch_n);
  const int64_t* __restrict__ keys = keys_all + b * batch_n;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lo = INT32_MAX, hi = INT32_MIN;
  for (int i = tid; i < n; i += kR8Threads) {
    int32_t kv;
    if (SF.keys_out) {                           // field b's id + its table offset
      const int64_t k64 = SF.col[b][i] + SF.off[b];
      SF.keys_out[b * (int64_t)batch_n + i] = k64;
      kv = (int32_t)k64;
    } else {
      kv = (int32_t)keys[i];
    }
    L.k[0][i] = (uint32_t)kv;
    L.v[0][i] = (uint16_t)i;
    lo = min(lo, kv);
    hi = max(hi, kv);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    lo = min(lo, __shfl_xor(lo, off, 64));
    hi = max(hi, __shfl_xor(hi, off, 64));
  }
  if (tid == 0) {
    L.kmin = INT32_MAX;
    L.kmax = INT32_MIN;
  }
  __syncthreads();
  if (lane == 0) {
    atomicMin(&L.kmin, lo);
    atomicMax(&L.kmax, hi);
  }
  __syncthreads();
  R8T(1);
  const uint32_t kmin = (uint32_t)L.kmin;
  const uint32_t span = n > 0 ? (uint32_t)L.kmax - kmin : 0u;
  int bits = 0;
  while (bits < 32 && (span >> bits) != 0u) ++bits;
  const int nch = (n + 63) >> 6;
  const int cpw = (nch + kR8Waves - 1) / kR8Waves;   // chunks of this wave: [wid*cpw, +cpw)
  const uint64_t lt = (1ull << lane) - 1ull;
  int cur = 0;
  for (int shift = 0; shift < bits; shift += 8) {
    for (int q = tid; q < 256 * kR8Waves; q += kR8Threads) L.hist[q] = 0;
    __syncthreads();                             // keys of the pass in place, counters zeroed
#pragma unroll 1
    for (int cc = 0; cc < cpw; ++cc) {           // rolled: a short code path (one pass of
      const int i = (wid * cpw + cc) * 64 + lane;  // one block runs cold in the I-cache)
      const bool valid = i < n;
      const uint32_t dd = valid ? ((L.k[cur][i] - kmin) >> shift) & 255u : 0u;
      rank_chunk8<kR8Waves>(dd, valid, lt, L.hist, wid, L.rank, i);
    }
    if (shift == 8) R8T(8);
    __syncthreads();
    scan_digit_counters<kR8Waves, kR8Threads>(L.hist, L.scan);
    __syncthreads();
    if (shift == 8) R8T(9);
#pragma unroll 1
    for (int cc = 0; cc < cpw; ++cc) {
      const int i = (wid * cpw + cc) * 64 + lane;
      if (i < n) {
        const uint32_t kv = L.k[cur][i];
        const int dst = L.hist[(int)(((kv - kmin) >> shift) & 255u) * kR8Waves + wid] + L.rank[i];
        L.k[cur ^ 1][dst] = kv;
        L.v[cur ^ 1][dst] = L.v[cur][i];
      }
    }
    cur ^= 1;
    if (shift == 8) R8T(10);
    __syncthreads();                             // offsets read before the next zeroing
    R8T(2 + shift / 8);
  }
  R8T(6);
  const uint32_t* __restrict__ ks = L.k[cur];
  const int per = (n + kR8Threads - 1) / kR8Threads;  // uniq / seg: one scan over runs of
  const int i0 = min(n, tid * per), i1 = min(n, i0 + per);   // per keys a thread
  int f = 0;
  for (int i = i0; i < i1; ++i) f += (i == 0 || ks[i - 1] != ks[i]) ? 1 : 0;
  int nu;
  int o = block_exclusive_scan(f, L.scan, &nu);
  const int64_t pos0 = b * (int64_t)batch_n;
  int32_t *perm, *uniq, *seg;
  int32_t voff;                                  // added to block-local positions
  if (status) {
    // the count is the whole message: relaxed agent-scope store and loads (an agent
    // release / acquire is buffer_wbl2 / buffer_inv on gfx950 — see step.hip, part_store)
    if (tid == 0) __hip_atomic_store(&status[b], nu + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (wid == 0) {
      int acc = 0;
      for (int64_t j0 = 0; j0 < b; j0 += 64) {
        const int64_t j = j0 + lane;
        int c = 0;
        if (j < b) {
          while ((c = __hip_atomic_load(&status[j], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT)) == 0)
            __builtin_amdgcn_s_sleep(1);
          c -= 1;
        }
        acc += wave_sum_i(c);
      }
      if (lane == 0) L.base = acc;
    }
    __syncthreads();
    perm = perm_all + pos0;
    uniq = uniq_all + L.base;
    seg = seg_all + L.base;
    voff = (int32_t)pos0;
  } else {
    perm = perm_all + pos0;
    uniq = uniq_all + pos0;
    seg = seg_all + b * (int64_t)(batch_n + 1);
    voff = 0;
  }
  for (int i = tid; i < n; i += kR8Threads) perm[i] = voff + L.v[cur][i];
  int32_t* __restrict__ pu = pu_all ? pu_all + pos0 : nullptr;   // chained only
  const int ubase = status ? L.base : 0;
  for (int i = i0; i < i1; ++i) {
    if (i == 0 || ks[i - 1] != ks[i]) {
      uniq[o] = (int32_t)ks[i];
      seg[o] = voff + i;
      ++o;
    }
    if (pu) pu[i] = ubase + o - 1;               // the segment of sorted position i
  }
  if (!status) {
    if (tid == 0) {
      seg[nu] = n;
      n_uniq_all[b] = nu;
    }
  } else {
    const int nblocks = (int)gridDim.x;
    if (tid == 0) {
      if (b == nblocks - 1) {
        seg[nu] = (int32_t)n_total;
        n_uniq_all[0] = L.base + nu;
      }
      // relaxed: this block's look-back loads have returned (their sum is in L.base)
      L.last = __hip_atomic_fetch_add(&status[nblocks], 1, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT) == nblocks - 1;
    }
    __syncthreads();
    if (L.last)                                  // every block is past its look-back
      for (int q = tid; q <= nblocks; q += kR8Threads) status[q] = 0;
  }
  R8T(7);
  R8C(13);
}

// Block-partitioned sort (keys in n_blocks blocks of block_n, every key of block b
// below every key of block b+1 — DeepFM's token keys, one block per field at its
// table offset): each block sorted in LDS by its own workgroup, then concatenated —
// the global stable sort, in two launches instead of a device-wide radix sort.
__global__ __launch_bounds__(256) void blocks_concat_kernel(
    const int32_t* __restrict__ perm_t, const int32_t* __restrict__ uniq_t,
    const int32_t* __restrict__ seg_t, const int32_t* __restrict__ nu_t, int64_t n,
    int block_n, int n_blocks, int32_t* __restrict__ perm, int32_t* __restrict__ uniq,
    int32_t* __restrict__ seg, int32_t* __restrict__ n_uniq) {
  const int b = blockIdx.x;
  int off = 0;
  for (int c = 0; c < b; ++c) off += nu_t[c];
  const int nu = nu_t[b];
  const int64_t base = (int64_t)b * block_n;
  const int nb = (int)min((int64_t)block_n, n - base);
  for (int i = threadIdx.x; i < nb; i += blockDim.x) perm[base + i] = (int32_t)base + perm_t[base + i];
  for (int i = threadIdx.x; i < nu; i += blockDim.x) {
    uniq[off + i] = uniq_t[base + i];
    seg[off + i] = (int32_t)base + seg_t[(int64_t)b * (block_n + 1) + i];
  }
  if (b == n_blocks - 1 && threadIdx.x == 0) {
    seg[off + nu] = (int32_t)n;
    n_uniq[0] = off + nu;
  }
}

// Two batched sorts in one launch (the user and the item keys of a chunk):
// workgroups [0, nbA) sort table A's batches, the rest table B's.
struct SortJob {
  const int64_t* keys; int64_t n_total; int batch_n; int nbits;
  int32_t *perm, *uniq, *seg, *n_uniq;
};

__global__ __launch_bounds__(kSortThreads) void segsort_lds2_kernel(SortJob A, SortJob B,
                                                                    int64_t nbA) {
  __shared__ SortLds L;
  const bool a = (int64_t)blockIdx.x < nbA;
  const SortJob& J = a ? A : B;
  segsort_lds_batch(J.keys, J.n_total, J.batch_n, J.nbits, J.perm, J.uniq, J.seg, J.n_uniq,
                    a ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - nbA, L);
}

// Same algorithm, global ping-pong buffers, processed in chunks of
// kSortThreads*kIpt with running offsets (any n up to INT32_MAX).
__global__ __launch_bounds__(kSortThreads) void segsort_global_kernel(
    const int64_t* __restrict__ keys_all, int64_t n_total, int batch_n, int nbits,
    int32_t* __restrict__ perm_all, int32_t* __restrict__ uniq_all,
    int32_t* __restrict__ seg_all, int32_t* __restrict__ n_uniq_all, int32_t* __restrict__ ws) {
  __shared__ int scan_lds[kSortThreads / 64 + 1];
  const int64_t b = blockIdx.x;
  const int n = (int)min((int64_t)batch_n, n_total - b * batch_n);
  const int64_t* __restrict__ keys = keys_all + b * batch_n;
  int32_t* __restrict__ perm = perm_all + b * batch_n;
  int32_t* __restrict__ uniq = uniq_all + b * batch_n;
  int32_t* __restrict__ seg = seg_all + b * (batch_n + 1);
  int32_t* __restrict__ n_uniq = n_uniq_all + b;
  int32_t* kA = ws + b * 4 * (int64_t)batch_n;
  int32_t* vA = kA + batch_n;
  int32_t* kB = vA + batch_n;
  int32_t* vB = kB + batch_n;
  for (int i = threadIdx.x; i < n; i += kSortThreads) {
    kA[i] = (int32_t)keys[i];
    vA[i] = i;
  }
  __syncthreads();
  int32_t *ks = kA, *vs = vA, *kd = kB, *vd = vB;
  constexpr int CH = kSortThreads * kIpt;
  for (int bit = 0; bit < nbits; ++bit) {
    // total zeros
    int zloc = 0;
    for (int i = threadIdx.x; i < n; i += kSortThreads) zloc += ((ks[i] >> bit) & 1) ? 0 : 1;
    int Z;
    (void)block_exclusive_scan(zloc, scan_lds, &Z);
    int zrun = 0;  // zeros in earlier chunks
    for (int c0 = 0; c0 < n; c0 += CH) {
      const int lo = c0 + threadIdx.x * kIpt;
      const int hi = min(n, lo + kIpt);
      int z = 0;
      for (int i = lo; i < hi; ++i) z += ((ks[i] >> bit) & 1) ? 0 : 1;
      int zc;
      const int ez = block_exclusive_scan(z, scan_lds, &zc);
      int zb = zrun + ez;
      for (int i = lo; i < hi; ++i) {
        const int32_t kv = ks[i];
        const int one = (kv >> bit) & 1;
        const int dst = one ? (Z + (i - zb)) : zb;
        kd[dst] = kv;
        vd[dst] = vs[i];
        zb += 1 - one;
      }
      zrun += zc;
    }
    __threadfence_block();
    __syncthreads();
    int32_t* t;
    t = ks; ks = kd; kd = t;
    t = vs; vs = vd; vd = t;
  }
  for (int i = threadIdx.x; i < n; i += kSortThreads) perm[i] = vs[i];
  __syncthreads();
  emit_segments(ks, n, uniq, seg, n_uniq, scan_lds);
}

// ---------------------------------------------------------------------------
// Large single-batch sorts (n > kLdsMax: the autograd paths of the context and
// sequential models group 10^5..10^6 contributions per step). Device-wide
// stable LSD radix sort, 5-bit digits, one tile of kRadixTile keys per block:
//   upsweep   per-tile digit histogram            -> hist[digit * n_tiles + tile]
//   scan      exclusive scan of hist (digit-major) -> global destination bases
//   downsweep stable in-tile ranking (blocked layout, per-thread digit counts
//             scanned digit-major in LDS) -> scatter of (key, index)
// then segments: per-tile head-flag counts -> scan -> uniq / seg writes.
constexpr int kRadixThreads = 256;
constexpr int kRadixIpt = 8;
constexpr int kRadixTile = kRadixThreads * kRadixIpt;
constexpr int kRadixBits = 5;     // digit width: 5 passes for 25-bit key spaces (was 4 bits, 7)
constexpr int kRadixBins = 1 << kRadixBits;

__global__ __launch_bounds__(kRadixThreads) void radix_init_kernel(
    const int64_t* __restrict__ keys, int n, int32_t* __restrict__ k32, int32_t* __restrict__ v32) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    k32[i] = (int32_t)keys[i];
    v32[i] = i;
  }
}

// per-thread digit counts of the thread's kRadixIpt consecutive keys -> cnt[bin][t]
__device__ __forceinline__ void tile_counts(const int32_t* __restrict__ k, int n, int base,
                                            int shift, int* cnt, int32_t* my, int* nmy) {
  const int t = threadIdx.x;
  int c[kRadixBins];
#pragma unroll
  for (int b = 0; b < kRadixBins; ++b) c[b] = 0;
  int m = 0;
#pragma unroll
  for (int j = 0; j < kRadixIpt; ++j) {
    const int i = base + t * kRadixIpt + j;
    if (i < n) {
      my[j] = k[i];
      const int dg = (my[j] >> shift) & (kRadixBins - 1);
#pragma unroll
      for (int b = 0; b < kRadixBins; ++b) c[b] += (dg == b) ? 1 : 0;
      ++m;
    }
  }
#pragma unroll
  for (int b = 0; b < kRadixBins; ++b) cnt[b * kRadixThreads + t] = c[b];
  *nmy = m;
}

__global__ __launch_bounds__(kRadixThreads) void radix_upsweep_kernel(
    const int32_t* __restrict__ k, int n, int shift, int n_tiles, int32_t* __restrict__ hist) {
  __shared__ int cnt[kRadixBins * kRadixThreads];
  int32_t my[kRadixIpt];
  int nmy;
  tile_counts(k, n, blockIdx.x * kRadixTile, shift, cnt, my, &nmy);
  __syncthreads();
  if (threadIdx.x < kRadixBins) {
    int s = 0;
    for (int t = 0; t < kRadixThreads; ++t) s += cnt[threadIdx.x * kRadixThreads + t];
    hist[threadIdx.x * n_tiles + blockIdx.x] = s;
  }
}

// exclusive scan of a[0..m) in place (one block), a[m] = total
__global__ __launch_bounds__(1024) void scan_exclusive_kernel(int32_t* __restrict__ a, int m) {
  __shared__ int lds[1024 / 64 + 1];
  int run = 0;
  for (int c0 = 0; c0 < m; c0 += 1024) {
    const int i = c0 + threadIdx.x;
    const int x = i < m ? a[i] : 0;
    int tot;
    const int ex = block_exclusive_scan(x, lds, &tot);
    if (i < m) a[i] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) a[m] = run;
}

__global__ __launch_bounds__(kRadixThreads) void radix_downsweep_kernel(
    const int32_t* __restrict__ k, const int32_t* __restrict__ v, int n, int shift, int n_tiles,
    const int32_t* __restrict__ hist, int32_t* __restrict__ ko, int32_t* __restrict__ vo) {
  __shared__ int cnt[kRadixBins * kRadixThreads];
  __shared__ int part[kRadixThreads / 64 + 1];
  __shared__ int bin_start[kRadixBins];
  int32_t my[kRadixIpt];
  int nmy;
  const int base = blockIdx.x * kRadixTile;
  tile_counts(k, n, base, shift, cnt, my, &nmy);
  __syncthreads();
  // exclusive scan of cnt (thread-major, kRadixBins per thread: kRadixBins * kRadixThreads
  // entries), each thread's own bins serially, then a block scan of the thread totals
  const int t = threadIdx.x;
  int loc[kRadixBins];
  int s = 0;
#pragma unroll
  for (int j = 0; j < kRadixBins; ++j) {
    loc[j] = s;
    s += cnt[t * kRadixBins + j];
  }
  int tot;
  const int ex = block_exclusive_scan(s, part, &tot);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRadixBins; ++j) cnt[t * kRadixBins + j] = ex + loc[j];
  __syncthreads();
  if (t < kRadixBins) bin_start[t] = cnt[t * kRadixThreads];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kRadixIpt; ++j) {
    if (j < nmy) {
      const int dg = (my[j] >> shift) & (kRadixBins - 1);
      int before = 0;
#pragma unroll
      for (int q = 0; q < kRadixIpt; ++q) before += (q < j && ((my[q] >> shift) & (kRadixBins - 1)) == dg) ? 1 : 0;
      const int local = cnt[dg * kRadixThreads + t] - bin_start[dg] + before;
      const int dst = hist[dg * n_tiles + blockIdx.x] + local;
      const int i = base + t * kRadixIpt + j;
      ko[dst] = my[j];
      vo[dst] = v[i];
    }
  }
}

__global__ __launch_bounds__(kRadixThreads) void seg_count_kernel(const int32_t* __restrict__ k,
                                                                  int n,
                                                                  int32_t* __restrict__ tcnt) {
  __shared__ int part[kRadixThreads / 64 + 1];
  const int base = blockIdx.x * kRadixTile;
  int f = 0;
  for (int j = 0; j < kRadixIpt; ++j) {
    const int i = base + threadIdx.x * kRadixIpt + j;
    if (i < n) f += (i == 0 || k[i - 1] != k[i]) ? 1 : 0;
  }
  int tot;
  (void)block_exclusive_scan(f, part, &tot);
  if (threadIdx.x == 0) tcnt[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kRadixThreads) void seg_write_kernel(
    const int32_t* __restrict__ k, int n, int n_tiles, const int32_t* __restrict__ tbase,
    int32_t* __restrict__ uniq, int32_t* __restrict__ seg, int32_t* __restrict__ n_uniq) {
  __shared__ int part[kRadixThreads / 64 + 1];
  const int base = blockIdx.x * kRadixTile;
  int f = 0;
  for (int j = 0; j < kRadixIpt; ++j) {
    const int i = base + threadIdx.x * kRadixIpt + j;
    if (i < n) f += (i == 0 || k[i - 1] != k[i]) ? 1 : 0;
  }
  int tot;
  int o = tbase[blockIdx.x] + block_exclusive_scan(f, part, &tot);
  for (int j = 0; j < kRadixIpt; ++j) {
    const int i = base + threadIdx.x * kRadixIpt + j;
    if (i < n && (i == 0 || k[i - 1] != k[i])) {
      uniq[o] = k[i];
      seg[o] = i;
      ++o;
    }
  }
  if (blockIdx.x == n_tiles - 1 && threadIdx.x == 0) {
    const int total = tbase[n_tiles];
    seg[total] = n;
    n_uniq[0] = total;
  }
}

static size_t radix_ws_bytes(int64_t n) {
  const int64_t tiles = (n + kRadixTile - 1) / kRadixTile;
  return (size_t)4 * (size_t)n * sizeof(int32_t) +
         (size_t)(kRadixBins * tiles + 1 + tiles + 1) * sizeof(int32_t) + 256;
}

static int radix_segment_sort(const int64_t* keys, int n, int nbits, int32_t* perm,
                              int32_t* uniq, int32_t* seg, int32_t* n_uniq, void* ws,
                              hipStream_t st) {
  const int tiles = (n + kRadixTile - 1) / kRadixTile;
  int32_t* kA = (int32_t*)ws;
  int32_t* vA = kA + n;
  int32_t* kB = vA + n;
  int32_t* vB = kB + n;
  int32_t* hist = vB + n;                       // kRadixBins * tiles + 1
  int32_t* tcnt = hist + kRadixBins * tiles + 1;  // tiles + 1
  int g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(radix_init_kernel, dim3(g), dim3(256), 0, st, keys, n, kA, vA);
  const int passes = nbits == 0 ? 0 : (nbits + kRadixBits - 1) / kRadixBits;
  for (int p = 0; p < passes; ++p) {
    const int shift = kRadixBits * p;
    hipLaunchKernelGGL(radix_upsweep_kernel, dim3(tiles), dim3(kRadixThreads), 0, st, kA, n,
                       shift, tiles, hist);
    hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(1024), 0, st, hist,
                       kRadixBins * tiles);
    hipLaunchKernelGGL(radix_downsweep_kernel, dim3(tiles), dim3(kRadixThreads), 0, st, kA, vA,
                       n, shift, tiles, hist, kB, vB);
    int32_t* t = kA; kA = kB; kB = t;
    t = vA; vA = vB; vB = t;
  }
  {
    const int rc = hip_status(
        hipMemcpyAsync(perm, vA, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, st),
        "mirec_segment_sort (perm copy)");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(seg_count_kernel, dim3(tiles), dim3(kRadixThreads), 0, st, kA, n, tcnt);
  hipLaunchKernelGGL(scan_exclusive_kernel, dim3(1), dim3(1024), 0, st, tcnt, tiles);
  hipLaunchKernelGGL(seg_write_kernel, dim3(tiles), dim3(kRadixThreads), 0, st, kA, n, tiles,
                     tcnt, uniq, seg, n_uniq);
  return launch_status("mirec_segment_sort (radix)");
}

// ---------------------------------------------------------------------------
// Device-wide sort in few launches ("onesweep" form): one launch builds every pass's
// global digit histogram (8-bit digits: ceil(bits / 8) passes, 3 for a 3 M-row table
// instead of 5 five-bit passes of upsweep + scan + downsweep), one launch per pass ranks
// a 2,048-key tile stably in LDS (the ballot ranking of segsort_radix8_kernel) and finds
// its digit offsets among the tiles by decoupled look-back, and one launch emits the
// segments (with pos_seg) by a look-back scan of the run heads. 2 + passes launches,
// against 5 x 3 + 5. Same perm / uniq / seg / n_uniq (stable sort: unique).
//
// status (int32, zero before the first call, left zero: the last block of each launch
// zeroes what that launch used): hist [kOsMaxPasses][256] | look-back words [passes]
// [tiles][256] | segment look-back words [tiles] | tickets [kOsMaxPasses + 1]. A look-back
// word holds 1 << 30 | the tile's own count; a tile sums its predecessors' words
// (lookback.h).
constexpr int kOsThreads = 512;
constexpr int kOsWaves = kOsThreads / 64;
constexpr int kOsTile = 2048;
constexpr int kOsIpt = kOsTile / kOsThreads;       // keys per thread (loads)
constexpr int kOsChunks = kOsTile / 64 / kOsWaves;  // 64-key chunks per wave
constexpr int kOsMaxPasses = 4;

__host__ __device__ inline int64_t os_tiles(int64_t n) { return (n + kOsTile - 1) / kOsTile; }
__host__ __device__ inline int64_t os_status_words(int64_t n) {
  const int64_t t = os_tiles(n);
  return (int64_t)kOsMaxPasses * 256 + (int64_t)kOsMaxPasses * t * 256 + t + kOsMaxPasses + 1;
}

__global__ __launch_bounds__(kOsThreads) void os_hist_kernel(
    const int64_t* __restrict__ keys, int n, int passes, int32_t* __restrict__ k32,
    int32_t* __restrict__ v32, uint32_t* __restrict__ hist) {
  __shared__ int h[kOsMaxPasses][256];
  for (int q = threadIdx.x; q < kOsMaxPasses * 256; q += kOsThreads) (&h[0][0])[q] = 0;
  __syncthreads();
  const int base = blockIdx.x * kOsTile;
#pragma unroll
  for (int j = 0; j < kOsIpt; ++j) {
    const int i = base + j * kOsThreads + threadIdx.x;
    if (i < n) {
      const uint32_t kv = (uint32_t)keys[i];
      k32[i] = (int32_t)kv;
      v32[i] = i;
      for (int p = 0; p < passes; ++p) atomicAdd(&h[p][(kv >> (8 * p)) & 255u], 1);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < passes * 256; q += kOsThreads) {
    const int c = (&h[0][0])[q];
    if (c) __hip_atomic_fetch_add(hist + q, (uint32_t)c, __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct OsPassLds {
  uint32_t k[kOsTile];
  int32_t v[kOsTile];
  int cnt[256 * kOsWaves];           // [digit][wave] counts, then their offsets in the tile
  uint16_t rank[kOsTile];
  int gbase[256];                    // global start of each digit (this pass)
  int tstart[257];                   // start of each digit inside the tile
  int scan[kOsWaves + 1];
  uint32_t half[256];
  int last;
};

__global__ __launch_bounds__(kOsThreads) void os_pass_kernel(
    const int32_t* __restrict__ kin, const int32_t* __restrict__ vin, int n, int shift,
    int64_t tiles, uint32_t* __restrict__ hist_p, uint32_t* __restrict__ look_p,
    uint32_t* __restrict__ ticket_p, int32_t* __restrict__ kout, int32_t* __restrict__ vout) {
  __shared__ OsPassLds L;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t tile = blockIdx.x;
  const int base = (int)(tile * kOsTile);
  const int tn = min(kOsTile, n - base);
#pragma unroll
  for (int j = 0; j < kOsIpt; ++j) {
    const int i = j * kOsThreads + tid;
    if (i < tn) {
      L.k[i] = (uint32_t)kin[base + i];
      L.v[i] = vin[base + i];
    }
  }
  for (int q = tid; q < 256 * kOsWaves; q += kOsThreads) L.cnt[q] = 0;
  // the pass's global digit starts: an exclusive scan of its histogram
  {
    const int c = tid < 256 ? (int)hist_p[tid] : 0;
    int tot;
    const int ex = block_exclusive_scan(c, L.scan, &tot);
    if (tid < 256) L.gbase[tid] = ex;
  }
  __syncthreads();
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int cc = 0; cc < kOsChunks; ++cc) {       // wave wid owns chunks [wid * kOsChunks, ..)
    const int i = (wid * kOsChunks + cc) * 64 + lane;
    const bool valid = i < tn;
    const uint32_t dd = valid ? (L.k[i] >> shift) & 255u : 0u;
    rank_chunk8<kOsWaves>(dd, valid, lt, L.cnt, wid, L.rank, i);
  }
  __syncthreads();
  scan_digit_counters<kOsWaves, kOsThreads>(L.cnt, L.scan);   // offsets inside the tile
  __syncthreads();
  if (tid < 256) L.tstart[tid] = L.cnt[tid * kOsWaves];
  if (tid == 0) L.tstart[256] = tn;
  __syncthreads();
  if (tid < 256)                                 // digit tid: this tile's count
    os_store(look_p + tile * 256 + tid,
             kOsFlagA | (uint32_t)(L.tstart[tid + 1] - L.tstart[tid]));
  {                                              // the counts of the tiles before: thread
    const int dg = tid & 255, h = tid >> 8;      // (digit, half) sums every other tile
    const uint32_t part = os_sum_before(look_p + dg, tile, 256, h, kOsThreads / 256);
    if (h == 1) L.half[dg] = part;
    __syncthreads();
    if (h == 0)                                  // + the key's offset inside the tile
      L.gbase[dg] += (int)(part + L.half[dg]) - L.tstart[dg];
  }
  __syncthreads();
#pragma unroll
  for (int cc = 0; cc < kOsChunks; ++cc) {
    const int i = (wid * kOsChunks + cc) * 64 + lane;
    if (i < tn) {
      const uint32_t kv = L.k[i];
      const int dd = (int)((kv >> shift) & 255u);
      const int dst = L.gbase[dd] + L.cnt[dd * kOsWaves + wid] + L.rank[i];
      kout[dst] = (int32_t)kv;
      vout[dst] = L.v[i];
    }
  }
  // this pass's histogram and look-back words, zeroed by its last block
  os_cleanup(ticket_p, look_p, tiles * 256, &L.last);
  if (L.last)
    for (int q = tid; q < 256; q += kOsThreads) hist_p[q] = 0u;
}

__global__ __launch_bounds__(kOsThreads) void os_seg_kernel(
    const int32_t* __restrict__ k, int n, int64_t tiles, uint32_t* __restrict__ look,
    uint32_t* __restrict__ ticket, int32_t* __restrict__ uniq, int32_t* __restrict__ seg,
    int32_t* __restrict__ n_uniq, int32_t* __restrict__ pos_seg) {
  __shared__ int scan[kOsWaves + 1];
  __shared__ int prefix;
  __shared__ int last;
  const int64_t tile = blockIdx.x;
  const int base = (int)(tile * kOsTile);
  const int i0 = base + threadIdx.x * kOsIpt;      // blocked: kOsIpt consecutive keys
  int32_t kk[kOsIpt];
  int f = 0;
#pragma unroll
  for (int j = 0; j < kOsIpt; ++j) {
    const int i = i0 + j;
    kk[j] = i < n ? k[i] : 0;
    if (i < n) f += (i == 0 || k[i - 1] != kk[j]) ? 1 : 0;
  }
  int tot;
  const int ex = block_exclusive_scan(f, scan, &tot);
  if (threadIdx.x == 0) os_store(look + tile, kOsFlagA | (uint32_t)tot);
  {                                              // run heads of the tiles before this one
    const uint32_t part = os_sum_before(look, tile, 1, threadIdx.x, kOsThreads);
    int all;
    (void)block_exclusive_scan((int)part, scan, &all);
    if (threadIdx.x == 0) {
      prefix = all;
      if (tile == tiles - 1) {
        seg[all + tot] = n;
        n_uniq[0] = (int32_t)(all + tot);
      }
    }
  }
  __syncthreads();
  int o = prefix + ex;
#pragma unroll
  for (int j = 0; j < kOsIpt; ++j) {
    const int i = i0 + j;
    if (i < n) {
      if (i == 0 || k[i - 1] != kk[j]) {
        uniq[o] = kk[j];
        seg[o] = i;
        ++o;
      }
      if (pos_seg) pos_seg[i] = o - 1;
    }
  }
  os_cleanup(ticket, look, tiles, &last);
}

}  // namespace mirec

using namespace mirec;

extern "C" size_t mirec_segment_sort_workspace_size(int64_t n, int64_t key_space) {
  (void)key_space;
  if (n <= kLdsMax) return 256;
  return radix_ws_bytes(n);
}

extern "C" int mirec_segment_sort_batched(const int64_t* keys, int64_t n, int64_t batch_n,
                                          int64_t key_space, int32_t* perm, int32_t* uniq,
                                          int32_t* seg, int32_t* n_uniq_dev, void* ws,
                                          size_t ws_bytes, void* stream) {
  if (n < 0 || key_space <= 0 || key_space > INT32_MAX || n > INT32_MAX || batch_n < 0 ||
      !seg || !n_uniq_dev || (n > 0 && (!keys || !perm || !uniq || batch_n == 0))) {
    set_error("mirec_segment_sort: bad arguments");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
  const int nb = nbits_for(key_space);
  if (n == 0) {  // one empty batch: seg[0] = 0, n_uniq = 0
    hipLaunchKernelGGL(segsort_lds_kernel, dim3(1), dim3(kSortThreads), 0, st, keys, (int64_t)0,
                       1, nb, perm, uniq, seg, n_uniq_dev);
    return launch_status("mirec_segment_sort");
  }
  const int64_t n_batches = (n + batch_n - 1) / batch_n;
  if (n_batches == 1 && n > kLdsMax) {
    if (!ws || ws_bytes < radix_ws_bytes(n)) {
      set_error("mirec_segment_sort: workspace %zu < %zu", ws_bytes, radix_ws_bytes(n));
      return -1;
    }
    return radix_segment_sort(keys, (int)n, nb, perm, uniq, seg, n_uniq_dev, ws, st);
  }
  if (batch_n <= kLdsMax) {
    hipLaunchKernelGGL(segsort_lds_kernel, dim3((unsigned)n_batches), dim3(kSortThreads), 0, st,
                       keys, n, (int)batch_n, nb, perm, uniq, seg, n_uniq_dev);
  } else {
    const size_t need = (size_t)4 * (size_t)(n_batches * batch_n) * sizeof(int32_t);
    if (!ws || ws_bytes < need) {
      set_error("mirec_segment_sort: workspace %zu < %zu", ws_bytes, need);
      return -1;
    }
    hipLaunchKernelGGL(segsort_global_kernel, dim3((unsigned)n_batches), dim3(kSortThreads), 0,
                       st, keys, n, (int)batch_n, nb, perm, uniq, seg, n_uniq_dev,
                       (int32_t*)ws);
  }
  return launch_status("mirec_segment_sort");
}

extern "C" size_t mirec_segment_sort_blocks_workspace_size(int64_t n, int64_t block_n) {
  if (n <= 0 || block_n <= 0) return 256;
  const int64_t nb = (n + block_n - 1) / block_n;
  return (size_t)(2 * nb * block_n + nb * (block_n + 1) + nb) * sizeof(int32_t) + 256;
}

extern "C" int mirec_segment_sort_blocks(const int64_t* keys, int64_t n, int64_t block_n,
                                         int64_t key_space, int32_t* perm, int32_t* uniq,
                                         int32_t* seg, int32_t* n_uniq_dev, void* ws,
                                         size_t ws_bytes, void* stream) {
  if (n <= 0 || block_n <= 0 || block_n > kLdsMax || key_space <= 0 ||
      key_space > INT32_MAX || n > INT32_MAX || !keys || !perm || !uniq || !seg || !n_uniq_dev) {
    set_error("mirec_segment_sort_blocks: bad arguments (0 < block_n <= %d)", kLdsMax);
    return -1;
  }
  if (!ws || ws_bytes < mirec_segment_sort_blocks_workspace_size(n, block_n)) {
    set_error("mirec_segment_sort_blocks: workspace too small");
    return -1;
  }
  const int64_t nb = (n + block_n - 1) / block_n;
  int32_t* perm_t = (int32_t*)ws;
  int32_t* uniq_t = perm_t + nb * block_n;
  int32_t* seg_t = uniq_t + nb * block_n;
  int32_t* nu_t = seg_t + nb * (block_n + 1);
  const int nbits = nbits_for(key_space);
  hipStream_t st = (hipStream_t)stream;
  if (block_n <= kR8Max)       // 8-bit digits over the block's key span
    hipLaunchKernelGGL(segsort_radix8_kernel, dim3((unsigned)nb), dim3(kR8Threads), 0, st, keys,
                       n, (int)block_n, perm_t, uniq_t, seg_t, nu_t, (int32_t*)nullptr,
                       (int32_t*)nullptr, SortFields{});
  else
    hipLaunchKernelGGL(segsort_lds_kernel, dim3((unsigned)nb), dim3(kSortThreads), 0, st, keys,
                       n, (int)block_n, nbits, perm_t, uniq_t, seg_t, nu_t);
  hipLaunchKernelGGL(blocks_concat_kernel, dim3((unsigned)nb), dim3(256), 0, st, perm_t, uniq_t,
                     seg_t, nu_t, n, (int)block_n, (int)nb, perm, uniq, seg, n_uniq_dev);
  return launch_status("mirec_segment_sort_blocks");
}

extern "C" int mirec_segment_sort_blocks_chained(const int64_t* keys, int64_t n,
                                                 int64_t block_n, int64_t key_space,
                                                 int32_t* perm, int32_t* uniq, int32_t* seg,
                                                 int32_t* n_uniq_dev, int32_t* status,
                                                 int64_t n_status, int32_t* pos_seg,
                                                 void* stream) {
  if (n <= 0 || block_n <= 0 || block_n > kR8Max || key_space <= 0 || key_space > INT32_MAX ||
      n > INT32_MAX || !keys || !perm || !uniq || !seg || !n_uniq_dev || !status) {
    set_error("mirec_segment_sort_blocks_chained: bad arguments (0 < block_n <= %d)", kR8Max);
    return -1;
  }
  const int64_t nb = (n + block_n - 1) / block_n;
  if (nb > kChainMaxBlocks || n_status < nb + 1) {
    set_error("mirec_segment_sort_blocks_chained: %lld blocks need status[%lld] (at most %d "
              "blocks)", (long long)nb, (long long)(nb + 1), kChainMaxBlocks);
    return -1;
  }
  hipLaunchKernelGGL(segsort_radix8_kernel, dim3((unsigned)nb), dim3(kR8Threads), 0,
                     (hipStream_t)stream, keys, n, (int)block_n, perm, uniq, seg, n_uniq_dev,
                     status, pos_seg, SortFields{});
  return launch_status("mirec_segment_sort_blocks_chained");
}

extern "C" int mirec_segment_sort_fields_chained(const int64_t* const* cols,
                                                 const int64_t* offsets, int32_t n_fields,
                                                 int64_t B, int64_t key_space, int64_t* keys_out,
                                                 int32_t* perm, int32_t* uniq, int32_t* seg,
                                                 int32_t* n_uniq_dev, int32_t* status,
                                                 int64_t n_status, int32_t* pos_seg,
                                                 void* stream) {
  if (n_fields <= 0 || n_fields > kSortFields || B <= 0 || B > kR8Max || key_space <= 0 ||
      key_space > INT32_MAX || !cols || !offsets || !keys_out || !perm || !uniq || !seg ||
      !n_uniq_dev || !status || n_status < n_fields + 1) {
    set_error("mirec_segment_sort_fields_chained: bad arguments (1..%d fields of 1..%d keys)",
              kSortFields, kR8Max);
    return -1;
  }
  SortFields SF;
  memset(&SF, 0, sizeof(SF));
  for (int f = 0; f < n_fields; ++f) {
    if (!cols[f]) {
      set_error("mirec_segment_sort_fields_chained: field %d has no column", f);
      return -1;
    }
    SF.col[f] = cols[f];
    SF.off[f] = offsets[f];
  }
  SF.keys_out = keys_out;
  hipLaunchKernelGGL(segsort_radix8_kernel, dim3((unsigned)n_fields), dim3(kR8Threads), 0,
                     (hipStream_t)stream, (const int64_t*)keys_out, (int64_t)n_fields * B, (int)B,
                     perm, uniq, seg, n_uniq_dev, status, pos_seg, SF);
  return launch_status("mirec_segment_sort_fields_chained");
}

extern "C" int64_t mirec_segment_sort_onesweep_status_words(int64_t n) {
  return n > 0 ? os_status_words(n) : 0;
}

extern "C" int mirec_segment_sort_onesweep(const int64_t* keys, int64_t n, int64_t key_space,
                                           int32_t* perm, int32_t* uniq, int32_t* seg,
                                           int32_t* n_uniq_dev, int32_t* pos_seg, void* ws,
                                           size_t ws_bytes, int32_t* status, int64_t n_status,
                                           void* stream) {
  if (n <= 0 || n > (int64_t)kOsVal || key_space <= 0 || key_space > INT32_MAX || !keys ||
      !perm || !uniq || !seg || !n_uniq_dev || !status) {
    set_error("mirec_segment_sort_onesweep: bad arguments (0 < n < 2^30)");
    return -1;
  }
  if (n_status < os_status_words(n) || !ws || ws_bytes < (size_t)4 * (size_t)n * 4) {
    set_error("mirec_segment_sort_onesweep: status (%lld words) or workspace too small",
              (long long)os_status_words(n));
    return -1;
  }
  const int nbits = nbits_for(key_space);
  const int passes = nbits == 0 ? 1 : (nbits + 7) / 8;
  const int64_t tiles = os_tiles(n);
  uint32_t* hist = (uint32_t*)status;
  uint32_t* look = hist + kOsMaxPasses * 256;
  uint32_t* slook = look + (int64_t)kOsMaxPasses * tiles * 256;
  uint32_t* tickets = slook + tiles;
  int32_t* kA = (int32_t*)ws;
  int32_t* vA = kA + n;
  int32_t* kB = vA + n;
  int32_t* vB = kB + n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(os_hist_kernel, dim3((unsigned)tiles), dim3(kOsThreads), 0, st, keys,
                     (int)n, passes, kA, vA, hist);
  for (int p = 0; p < passes; ++p) {
    int32_t* vo = p == passes - 1 ? perm : vB;     // the last pass writes perm itself
    hipLaunchKernelGGL(os_pass_kernel, dim3((unsigned)tiles), dim3(kOsThreads), 0, st, kA, vA,
                       (int)n, 8 * p, tiles, hist + p * 256, look + (int64_t)p * tiles * 256,
                       tickets + p, kB, vo);
    int32_t* t = kA; kA = kB; kB = t;
    t = vA; vA = vB; vB = t;
  }
  hipLaunchKernelGGL(os_seg_kernel, dim3((unsigned)tiles), dim3(kOsThreads), 0, st, kA, (int)n,
                     tiles, slook, tickets + kOsMaxPasses, uniq, seg, n_uniq_dev, pos_seg);
  return launch_status("mirec_segment_sort_onesweep");
}

extern "C" int mirec_segment_sort(const int64_t* keys, int64_t n, int64_t key_space,
                                  int32_t* perm, int32_t* uniq, int32_t* seg,
                                  int32_t* n_uniq_dev, void* ws, size_t ws_bytes, void* stream) {
  return mirec_segment_sort_batched(keys, n, n > 0 ? n : 1, key_space, perm, uniq, seg,
                                    n_uniq_dev, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// Look-ahead lists of the deferred Adam (adam.hip): for consecutive batches b,
// b+1 of a chunk, out_b = uniq(b+1) \ uniq(b) in ascending order — the rows the
// next forward pass reads that step b's Adam does not touch (device code: ahead.h).
namespace mirec {

__global__ __launch_bounds__(kSortThreads) void uniq_ahead_diff_kernel(
    const int32_t* __restrict__ uniq, const int32_t* __restrict__ n_uniq, int64_t stride,
    int64_t n_batches, int32_t* __restrict__ out, int32_t* __restrict__ n_out) {
  __shared__ int32_t a_lds[kDiffLds];
  __shared__ int scan_lds[kSortThreads / 64 + 1];
  uniq_ahead_diff_batch(uniq, n_uniq, stride, n_batches, out, n_out, blockIdx.x, a_lds, scan_lds);
}

struct DiffJob {
  const int32_t* uniq; const int32_t* n_uniq; int64_t stride; int32_t* out; int32_t* n_out;
};

// Both tables' look-ahead lists in one launch: workgroups [0, nb) table A, the rest B.
__global__ __launch_bounds__(kSortThreads) void uniq_ahead_diff2_kernel(DiffJob A, DiffJob B,
                                                                        int64_t nb) {
  __shared__ int32_t a_lds[kDiffLds];
  __shared__ int scan_lds[kSortThreads / 64 + 1];
  const bool a = (int64_t)blockIdx.x < nb;
  const DiffJob& J = a ? A : B;
  uniq_ahead_diff_batch(J.uniq, J.n_uniq, J.stride, nb, J.out, J.n_out,
                        a ? (int64_t)blockIdx.x : (int64_t)blockIdx.x - nb, a_lds, scan_lds);
}

}  // namespace mirec

extern "C" int mirec_uniq_ahead_diff(const int32_t* uniq, const int32_t* n_uniq, int64_t stride,
                                     int64_t n_batches, int32_t* out, int32_t* n_out,
                                     void* stream) {
  if (!uniq || !n_uniq || !out || !n_out || stride <= 0 || n_batches < 0) {
    mirec::set_error("mirec_uniq_ahead_diff: bad arguments");
    return -1;
  }
  if (n_batches == 0) return 0;
  hipLaunchKernelGGL(mirec::uniq_ahead_diff_kernel, dim3((unsigned)n_batches),
                     dim3(mirec::kSortThreads), 0, (hipStream_t)stream, uniq, n_uniq, stride,
                     n_batches, out, n_out);
  return mirec::launch_status("mirec_uniq_ahead_diff");
}

// ---- both tables of a chunk (mirec_prepare_chunk, gather.hip): one sort launch
// and one look-ahead launch when both fit the LDS path, else the separate calls.
namespace mirec {
int sort_chunk_pair(const int64_t* ukeys, int64_t nU_keys, int64_t Bu, int64_t u_space,
                    int32_t* u_perm, int32_t* u_uniq, int32_t* u_seg, int32_t* u_nu,
                    const int64_t* ikeys, int64_t nI_keys, int64_t Bi, int64_t i_space,
                    int32_t* i_perm, int32_t* i_uniq, int32_t* i_seg, int32_t* i_nu,
                    int64_t n_batches, int32_t* u_ahead, int32_t* u_nah, int32_t* i_ahead,
                    int32_t* i_nah, void* ws, size_t ws_bytes, hipStream_t st) {
  if (Bu <= kLdsMax && Bi <= kLdsMax && u_space <= INT32_MAX && i_space <= INT32_MAX &&
      nU_keys == n_batches * Bu && nI_keys == n_batches * Bi && n_batches > 0) {
    SortJob A = {ukeys, nU_keys, (int)Bu, nbits_for(u_space), u_perm, u_uniq, u_seg, u_nu};
    SortJob B = {ikeys, nI_keys, (int)Bi, nbits_for(i_space), i_perm, i_uniq, i_seg, i_nu};
    hipLaunchKernelGGL(segsort_lds2_kernel, dim3((unsigned)(2 * n_batches)), dim3(kSortThreads),
                       0, st, A, B, n_batches);
    int rc = launch_status("mirec_prepare_chunk: sort");
    if (rc || !u_ahead) return rc;
    DiffJob DA = {u_uniq, u_nu, Bu, u_ahead, u_nah};
    DiffJob DB = {i_uniq, i_nu, Bi, i_ahead, i_nah};
    hipLaunchKernelGGL(uniq_ahead_diff2_kernel, dim3((unsigned)(2 * n_batches)),
                       dim3(kSortThreads), 0, st, DA, DB, n_batches);
    return launch_status("mirec_prepare_chunk: look-ahead");
  }
  int rc = mirec_segment_sort_batched(ukeys, nU_keys, Bu, u_space, u_perm, u_uniq, u_seg, u_nu,
                                      ws, ws_bytes, st);
  if (rc) return rc;
  rc = mirec_segment_sort_batched(ikeys, nI_keys, Bi, i_space, i_perm, i_uniq, i_seg, i_nu, ws,
                                  ws_bytes, st);
  if (rc || !u_ahead) return rc;
  rc = mirec_uniq_ahead_diff(u_uniq, u_nu, Bu, n_batches, u_ahead, u_nah, st);
  if (rc) return rc;
  return mirec_uniq_ahead_diff(i_uniq, i_nu, Bi, n_batches, i_ahead, i_nah, st);
}
}  // namespace mirec
