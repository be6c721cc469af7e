// K2 — fixed-order reduction of grouped contributions (the grouping: segsort.hip).
//
// Chunked segmented scatter-add (hot rows: a Zipf head row may own 10^4..10^5
// contributions, far too many for one wave to sum serially). Every segment is cut
// into pieces of CH = scat_chunk(d) positions counted from ITS OWN start, so a row's
// sum depends only on its own contributions and their order — not on where the row
// sits in the sorted array (a row-sharded owner's shorter array gives the one-process
// sums bit for bit). Work is dealt by absolute chunks of CH positions: the group of G
// lanes of chunk c sums every piece that STARTS in c (reading past c's end when the
// piece does) — the pieces of the segments that start in c, plus at most one later
// piece of the segment that started before c. A one-piece segment is written
// directly; a longer one leaves its first piece in tail[chunk of its start] and
// piece k in head[that chunk + k] (at most one of each per chunk), which the fixup
// kernel (owner: the block of the first boundary after the segment's start) adds in
// piece order. Deterministic, no float atomics.
#include "common.h"
#include "lookback.h"

namespace mirec {

// positions per chunk: short chunks for wide rows (more lane groups in flight),
// longer ones for narrow rows; the workspace is sized for the smallest
#ifndef MIREC_SCAT_NARROW_CH
#define MIREC_SCAT_NARROW_CH 8
#endif
// 8 positions per piece up to d = 16 (DeepFM tokens: C4 4.34 -> 4.54 M samples/s against 32)
__host__ __device__ __forceinline__ int scat_chunk(int d) {
  return d == 1 ? 8 : d <= 16 ? MIREC_SCAT_NARROW_CH : 32;
}
constexpr int kScatChunkMin = 8;

__device__ __forceinline__ int seg_of(const int32_t* __restrict__ seg, int nu, int p) {
  int lo = 0, hi = nu - 1;   // largest u with seg[u] <= p
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid] <= p) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// The piece rule, which every reduction kernel below follows (their outputs are bit for
// bit the same only because they do): the pieces of a segment [s0, e) are [s0 + k CH,
// min(e, s0 + (k + 1) CH)), counted from the segment's own start, and chunk [p0, p1) of
// the sorted array owns the pieces that START inside it. A one-piece segment's piece is
// final (written to the output row); a longer segment's first piece is a tail piece and
// its later ones head pieces (summed by the fixup kernel).
//
// With pos_seg (the segment of every sorted position) a lane resolves sorted position q
// against chunk [p0, p1) without a search: its perm, whether the chunk owns its piece,
// whether q starts / ends the piece, the piece's kind, and where a final piece goes.
// Out: pq = perm[q]; info = 1 owned | 2 piece start | 4 piece end | kind << 3; dst = the
// output row of a final piece, else the segment. All zero for q >= n or a piece not owned.
constexpr int kWinKindFinal = 0, kWinKindTail = 1, kWinKindHead = 2;
template <int CH>
__device__ __forceinline__ void window_resolve(int q, int p0, int p1, int n, int compact,
                                               const int32_t* perm, const int32_t* pos_seg,
                                               const int32_t* uniq, const int32_t* seg,
                                               int& pq, int& info, int& dst) {
  pq = info = dst = 0;
  if (q < n) {
    pq = perm[q];
    const int u = pos_seg[q];
    const int s0 = seg[u], e = seg[u + 1];
    const int ps = s0 + (q - s0) / CH * CH;
    if (ps >= p0 && ps < p1) {
      const int pe = min(e, ps + CH);
      const int kind = ps != s0 ? kWinKindHead : (e - s0 <= CH ? kWinKindFinal : kWinKindTail);
      info = 1 | (q == ps ? 2 : 0) | (q == pe - 1 ? 4 : 0) | (kind << 3);
      dst = kind == kWinKindFinal ? (compact ? u : uniq[u]) : u;
    }
  }
}

// The searching form (no pos_seg): the group of G lanes of chunk c finds the segment of
// p0 by binary search and walks the segments that start in the chunk — the piece rule
// above (window_resolve).
// PAIR (mirec_segment_reduce2_f32): a second, one-column source grouped by the same
// segments (DeepFM's first-order [V, 1] weights beside the [V, d] token rows) is summed
// by lane 0 of each group in the same pass, position by position in the same order as
// the one-column kernel; its pieces go to head1 / tail1.
template <int G, int DMAX, bool PAIR = false>
__global__ __launch_bounds__(256) void scatter_chunks_kernel(
    const float* __restrict__ rows, int d, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ uniq, const int32_t* __restrict__ seg,
    const int32_t* __restrict__ n_uniq_dev, float* __restrict__ dense, int64_t n_rows,
    float* __restrict__ head, float* __restrict__ tail, int32_t* __restrict__ tail_seg,
    int n_chunks, int compact, const float* __restrict__ rows1 = nullptr,
    float* __restrict__ dense1 = nullptr, float* __restrict__ head1 = nullptr,
    float* __restrict__ tail1 = nullptr) {
  const int nu = n_uniq_dev[0];
  const int n = seg[nu];
  const int lane = threadIdx.x & 63;
  const int gi = lane / G, l = lane % G;
  const int c = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64) * (64 / G) + gi;
  if (c >= n_chunks) return;
  const int CH = scat_chunk(d);
  const int p0 = c * CH;
  if (nu == 0 || p0 >= n) {
    if (l == 0) tail_seg[c] = -1;
    return;
  }
  const int p1 = min(n, p0 + CH);
  constexpr int MAXC = DMAX / G;    // columns per lane, d <= DMAX
  // sums positions [q0, q1) of one segment into acc (loads 4 positions ahead of the adds)
  float acc1 = 0.f;                         // PAIR: the one-column source (lane 0)
  auto piece = [&](int q0, int q1, float* acc) {
    int q = q0;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) acc[j] = 0.f;
    acc1 = 0.f;
    for (; q + 4 <= q1; q += 4) {
      int pr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) pr[t] = perm[q + t];
      float v[4][MAXC];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
          const int col = l + j * G;
          v[t][j] = col < d ? rows[(int64_t)pr[t] * d + col] : 0.f;
        }
      float v1[4];
      if (PAIR) {
#pragma unroll
        for (int t = 0; t < 4; ++t) v1[t] = l == 0 ? rows1[pr[t]] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int j = 0; j < MAXC; ++j) acc[j] += v[t][j];
      if (PAIR) {
#pragma unroll
        for (int t = 0; t < 4; ++t) acc1 += v1[t];
      }
    }
    for (; q < q1; ++q) {
      const float* r = rows + (int64_t)perm[q] * d;
#pragma unroll
      for (int j = 0; j < MAXC; ++j) {
        const int col = l + j * G;
        if (col < d) acc[j] += r[col];
      }
      if (PAIR && l == 0) acc1 += rows1[perm[q]];
    }
  };
  auto store1 = [&](float* dst) {
    if (PAIR && l == 0 && dst) *dst = acc1;
  };
  auto store = [&](float* dst, const float* acc, bool add) {
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
      const int col = l + j * G;
      if (dst && col < d) {
        if (add) dst[col] += acc[j]; else dst[col] = acc[j];
      }
    }
  };
  float acc[MAXC];
  int u = seg_of(seg, nu, p0);
  if (seg[u] < p0) {                       // the segment that started before this chunk
    const int s0 = seg[u], e = seg[u + 1];
    const int ps = s0 + (p0 - s0 + CH - 1) / CH * CH;   // its next piece start >= p0
    if (ps < p1 && ps < e) {
      piece(ps, min(e, ps + CH), acc);
      store(head + (int64_t)c * d, acc, false);
      store1(PAIR ? head1 + c : nullptr);
    }
    ++u;
  }
  int ts = -1;                              // the multi-piece segment starting here, if any
  for (; u < nu && seg[u] < p1; ++u) {     // the segments that start in this chunk
    const int s0 = seg[u], e = seg[u + 1];
    piece(s0, min(e, s0 + CH), acc);
    if (e - s0 <= CH) {
      const int64_t row = compact ? (int64_t)u : (int64_t)uniq[u];
      store((row >= 0 && row < n_rows) ? dense + row * d : nullptr, acc, !compact);
      store1(PAIR ? dense1 + u : nullptr);       // PAIR: compact outputs only
    } else {
      store(tail + (int64_t)c * d, acc, false);
      store1(PAIR ? tail1 + c : nullptr);
      ts = u;
    }
  }
  if (l == 0) tail_seg[c] = ts;            // the fixup's owner list: no search there
}

// Fixup of the multi-piece segments: the owner of boundary b is the segment that starts
// in chunk b - 1 and continues (tail_seg, written by the chunk kernel). Its sum is
// defined by 256 partial sums per column block of CW = d rounded up to a power of two
// columns: "thread" i (column cb + i % CW, kl = i / CW, KL = 256 / CW) sums
// [tail[b-1] if kl = 0] + head[b + kl] + head[b + kl + KL] + ..., and the column's sum
// is t = s_0 + s_1 + ... + s_{KL-1} in kl order — deterministic. One wave per boundary
// forms the 256 partial sums (four per lane, their loads in flight together), stages
// them in its LDS slice and folds them; four boundaries per workgroup. The one-column
// source of a pair uses the same rule with CW = 1 (KL = 256).
constexpr int kFixWaves = 4;
__global__ __launch_bounds__(64 * kFixWaves) void scatter_fixup_kernel(
    int d, const int32_t* __restrict__ uniq, const int32_t* __restrict__ seg,
    const int32_t* __restrict__ tail_seg, float* __restrict__ dense, int64_t n_rows,
    const float* __restrict__ head, const float* __restrict__ tail, int n_chunks, int compact,
    float* __restrict__ dense1 = nullptr, const float* __restrict__ head1 = nullptr,
    const float* __restrict__ tail1 = nullptr) {
  __shared__ float red[kFixWaves][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = 1 + (int)blockIdx.x * kFixWaves + w;           // this wave's boundary
  if (b >= n_chunks) return;
  const int u = tail_seg[b - 1];
  if (u < 0) return;
  const int CH = scat_chunk(d);
  const int s0 = seg[u], e = seg[u + 1];
  const int kend = b - 2 + (e - s0 + CH - 1) / CH;     // chunk holding its last piece's start
  const int64_t row = compact ? (int64_t)u : (int64_t)uniq[u];
  if (row < 0 || row >= n_rows) return;
  float* R = red[w];
  // partial sums of "threads" i = lane + 64 j over src (ld columns, CW, KL), into R
  auto partials = [&](const float* __restrict__ hs, const float* __restrict__ ts, int ld, int cb,
                      int CW, int KL) {
    float acc[4];
    int col[4], kl[4];
    // loads are unconditional (clamped to a valid address) and the term is selected
    // afterwards: loads under per-lane branches wait for each other
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = lane + 64 * j;
      col[j] = cb + i % CW;
      kl[j] = i / CW;
      const float tv = ts[(int64_t)(b - 1) * ld + min(col[j], ld - 1)];
      acc[j] = (kl[j] == 0 && col[j] < ld) ? tv : 0.f;
    }
    for (int r0 = 0; b + r0 * KL <= kend; r0 += 4) {   // four rounds' loads in flight
      float hv[4][4];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = min(b + kl[j] + (r0 + rr) * KL, kend);
          hv[rr][j] = hs[(int64_t)k * ld + min(col[j], ld - 1)];
        }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (col[j] < ld && b + kl[j] + (r0 + rr) * KL <= kend) acc[j] += hv[rr][j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) R[lane + 64 * j] = acc[j];
  };
  int cw = 1;
  while (cw < d && cw < 256) cw <<= 1;
  const int KL = 256 / cw;
  for (int cb = 0; cb < d; cb += cw) {
    partials(head, tail, d, cb, cw, KL);
    __builtin_amdgcn_wave_barrier();                // one wave: its LDS ops stay in order
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = lane + 64 * j;
      if (i < cw && cb + i < d) {
        float t = R[i];
        for (int z = 1; z < KL; ++z) t += R[z * cw + i];
        if (compact) dense[row * d + cb + i] = t; else dense[row * d + cb + i] += t;
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (dense1) {          // PAIR: the one-column source, as the d = 1 fixup sums it
    partials(head1, tail1, 1, 0, 1, 256);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      // partial sums without a term are +0: adding them in order only turns a -0 running
      // sum into +0, which one add of +0 does as well
      const int m = min(256, kend - b + 1);
      float t = R[0];
      for (int z = 1; z < m; ++z) t += R[z];
      if (m < 256) t += 0.f;
      dense1[row] = t;
    }
  }
}

// Narrow rows (2 <= d <= 16) with pos_seg (the segment of every sorted position, from
// the chained block sort): chunk c of CH = 8 sorted positions owns the same pieces as
// in scatter_chunks_kernel and sums them in the same order, so the outputs are bit for
// bit the same. No search and no serial walk over segments: the 16 lanes of a group each
// resolve one position of the window [p0, p0 + 2 CH) (window_resolve), every lane then
// loads its column of the 16 window rows at once and folds them in order.
template <bool PAIR>
__global__ __launch_bounds__(256) void scatter_window_kernel(
    const float* __restrict__ rows, int d, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ pos_seg, const int32_t* __restrict__ uniq,
    const int32_t* __restrict__ seg, const int32_t* __restrict__ n_uniq_dev,
    float* __restrict__ dense, int64_t n_rows, float* __restrict__ head,
    float* __restrict__ tail, int32_t* __restrict__ tail_seg, int n_chunks, int compact,
    const float* __restrict__ rows1, float* __restrict__ dense1, float* __restrict__ head1,
    float* __restrict__ tail1) {
  constexpr int G = 16, CH = 8, W = 2 * CH;
  const int nu = n_uniq_dev[0];
  const int n = seg[nu];
  const int lane = threadIdx.x & 63, gb = lane & ~(G - 1), l = lane & (G - 1);
  const int c = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G);
  if (c >= n_chunks) return;
  const int p0 = c * CH;
  if (nu == 0 || p0 >= n) {
    if (l == 0) tail_seg[c] = -1;
    return;
  }
  const int p1 = min(n, p0 + CH);
  // lane l resolves window position q = p0 + l
  int dst, info, pq;
  window_resolve<CH>(p0 + l, p0, p1, n, compact, perm, pos_seg, uniq, seg, pq, info, dst);
  // the multi-piece segment starting here (its first piece is a tail piece), if any
  const uint64_t tb = __ballot((info & 2) && (info >> 3) == kWinKindTail);
  const uint64_t gm = tb & (0xFFFFull << gb);
  const int tl = gm ? __builtin_ctzll(gm) : gb;
  const int tsu = __shfl(dst, tl, 64);
  if (l == 0) tail_seg[c] = gm ? tsu : -1;
  int pt[W], it[W], dt[W];
#pragma unroll
  for (int t = 0; t < W; ++t) {
    pt[t] = __shfl(pq, gb + t, 64);
    it[t] = __shfl(info, gb + t, 64);
    dt[t] = __shfl(dst, gb + t, 64);
  }
  // every lane loads all W rows (unowned positions read row pt = 0 of a valid position;
  // their terms are skipped below): loads under per-lane branches wait for each other
  float v[W], v1[W];
  const int lc = min(l, d - 1);
#pragma unroll
  for (int t = 0; t < W; ++t) {
    v[t] = rows[(int64_t)pt[t] * d + lc];
    if (PAIR) v1[t] = rows1[pt[t]];
  }
  float acc = 0.f, acc1 = 0.f;
#pragma unroll
  for (int t = 0; t < W; ++t) {
    if (!(it[t] & 1)) continue;
    acc = ((it[t] & 2) ? 0.f : acc) + v[t];
    if (PAIR) acc1 = ((it[t] & 2) ? 0.f : acc1) + v1[t];
    if (!(it[t] & 4)) continue;
    const int kind = it[t] >> 3;
    if (kind == kWinKindFinal) {
      const int64_t row = dt[t];
      if (l < d && row >= 0 && row < n_rows) {
        if (compact) dense[row * d + l] = acc; else dense[row * d + l] += acc;
      }
      if (PAIR && l == 0) dense1[dt[t]] = acc1;
    } else {
      float* out = (kind == kWinKindTail ? tail : head) + (int64_t)c * d;
      if (l < d) out[l] = acc;
      if (PAIR && l == 0) (kind == kWinKindTail ? tail1 : head1)[c] = acc1;
    }
  }
}

// Wide rows (16 < d <= 256) with pos_seg: chunk c of CH = 32 sorted positions owns the
// same pieces as scatter_chunks_kernel and sums them in the same order (bit for bit).
// One wave per chunk: lane l resolves window position p0 + l of [p0, p0 + 64)
// (window_resolve); then the wave walks the window in order, eight positions' row loads
// in flight at a time — position t's perm and flags come from lane t by readlane, so the
// walk is uniform (scalar branches) and every row read is one coalesced access of the
// lanes' columns (l, l + 64, ...).
template <int MAXC>
__global__ __launch_bounds__(256) void scatter_wide_window_kernel(
    const float* __restrict__ rows, int d, const int32_t* __restrict__ perm,
    const int32_t* __restrict__ pos_seg, const int32_t* __restrict__ uniq,
    const int32_t* __restrict__ seg, const int32_t* __restrict__ n_uniq_dev,
    float* __restrict__ dense, int64_t n_rows, float* __restrict__ head,
    float* __restrict__ tail, int32_t* __restrict__ tail_seg, int n_chunks, int compact) {
  constexpr int CH = 32, W = 64;
  const int nu = n_uniq_dev[0];
  const int n = seg[nu];
  const int lane = threadIdx.x & 63;
  const int c = __builtin_amdgcn_readfirstlane(
      (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6));
  if (c >= n_chunks) return;
  const int p0 = c * CH;
  if (nu == 0 || p0 >= n) {
    if (lane == 0) tail_seg[c] = -1;
    return;
  }
  const int p1 = min(n, p0 + CH);
  int dst, info, pq;
  window_resolve<CH>(p0 + lane, p0, p1, n, compact, perm, pos_seg, uniq, seg, pq, info, dst);
  const uint64_t tb = __ballot((info & 2) && (info >> 3) == kWinKindTail);
  const int tsu = tb ? __builtin_amdgcn_readlane(dst, __builtin_ctzll(tb)) : -1;
  if (lane == 0) tail_seg[c] = tsu;
  int col[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) col[j] = min(lane + 64 * j, d - 1);
  float acc[MAXC];
#pragma unroll
  for (int j = 0; j < MAXC; ++j) acc[j] = 0.f;
  for (int t0 = 0; t0 < W; t0 += 8) {
    int it[8], pt[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      it[j] = __builtin_amdgcn_readlane(info, t0 + j);
      pt[j] = __builtin_amdgcn_readlane(pq, t0 + j);
    }
    float v[8][MAXC];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
      for (int cc = 0; cc < MAXC; ++cc)
        v[j][cc] = (it[j] & 1) ? rows[(int64_t)pt[j] * d + col[cc]] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (!(it[j] & 1)) continue;
#pragma unroll
      for (int cc = 0; cc < MAXC; ++cc) acc[cc] = ((it[j] & 2) ? 0.f : acc[cc]) + v[j][cc];
      if (!(it[j] & 4)) continue;
      const int kind = it[j] >> 3;
      const int dt = __builtin_amdgcn_readlane(dst, t0 + j);
      if (kind == kWinKindFinal) {
        const int64_t row = dt;
        if (row >= 0 && row < n_rows) {
#pragma unroll
          for (int cc = 0; cc < MAXC; ++cc) {
            const int cl = lane + 64 * cc;
            if (cl < d) {
              if (compact) dense[row * d + cl] = acc[cc]; else dense[row * d + cl] += acc[cc];
            }
          }
        }
      } else {
        float* out = (kind == kWinKindTail ? tail : head) + (int64_t)c * d;
#pragma unroll
        for (int cc = 0; cc < MAXC; ++cc) {
          const int cl = lane + 64 * cc;
          if (cl < d) out[cl] = acc[cc];
        }
      }
    }
  }
}

// Union of two reduced gradients (the deferred optimizer's second level, one table read
// by two autograd Functions): A = (uA[0..nA), rowsA), B = (uB[0..nB), rowsB), each
// ascending and distinct. Output: the union rows ascending, each row's sum formed as the
// second-level segment_reduce of [A's rows; B's rows] formed it — (0 + a) + b, 0 + a,
// 0 + b — where a_pre = 1 takes a as already carrying its leading 0 + (a previous
// merge's output): the same bits, with no sort of the concatenated keys and no reduce.
// Two launches: a stable merge of the key lists (A before B on equal keys) into the
// merged order, then the run heads (tile counts summed over the tiles before by
// look-back, lookback.h) with each head's one or two rows summed by a wave.
__device__ __forceinline__ int merge_lower(const int32_t* __restrict__ a, int n, int32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int merge_upper(const int32_t* __restrict__ a, int n, int32_t key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void merge_place_kernel(
    const int32_t* __restrict__ uA, const int32_t* __restrict__ nA_dev, int capA,
    const int32_t* __restrict__ uB, const int32_t* __restrict__ nB_dev, int capB,
    int32_t* __restrict__ mk, int32_t* __restrict__ ref) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nA = nA_dev[0], nB = nB_dev[0];
  if (i < capA) {
    if (i >= nA) return;
    const int32_t key = uA[i];
    const int pos = (int)i + merge_lower(uB, nB, key);
    mk[pos] = key;
    ref[pos] = (int32_t)i;
  } else if (i < (int64_t)capA + capB) {
    const int j = (int)(i - capA);
    if (j >= nB) return;
    const int32_t key = uB[j];
    const int pos = j + merge_upper(uA, nA, key);
    mk[pos] = key;
    ref[pos] = (int32_t)(0x80000000u | (uint32_t)j);
  }
}

constexpr int kMergeThreads = 256;
constexpr int kMergeIpt = 2;
constexpr int kMergeTile = kMergeThreads * kMergeIpt;   // merged positions per workgroup

// one output row's (up to two) source rows folded, V floats at column c
template <int V>
__device__ __forceinline__ void merge_fold(const float* __restrict__ s0,
                                           const float* __restrict__ s1, bool pre0, bool two,
                                           float* __restrict__ dst) {
#pragma unroll
  for (int e = 0; e < V; ++e) {
    float v = s0[e];
    if (!pre0) v = 0.f + v;
    if (two) v = v + s1[e];
    dst[e] = v;
  }
}

template <int V>
__global__ __launch_bounds__(kMergeThreads) void merge_compact_kernel(
    const int32_t* __restrict__ mk, const int32_t* __restrict__ ref,
    const int32_t* __restrict__ nA_dev, const int32_t* __restrict__ nB_dev,
    const float* __restrict__ rowsA, const float* __restrict__ rowsB, int d, int a_pre,
    int32_t* __restrict__ uniq_out, int32_t* __restrict__ n_out, float* __restrict__ rows_out,
    uint32_t* __restrict__ look, uint32_t* __restrict__ ticket) {
  __shared__ int scan[kMergeThreads / 64 + 1];
  __shared__ int hp[kMergeTile];                  // merged position of each run head
  __shared__ int h0[kMergeTile], h1[kMergeTile];  // each head's source rows
  __shared__ int prefix, n_heads, last;
  const int m = nA_dev[0] + nB_dev[0];
  const int64_t tile = blockIdx.x;
  const int base = (int)(tile * kMergeTile);
  const int i0 = base + threadIdx.x * kMergeIpt;
  int f = 0;
#pragma unroll
  for (int j = 0; j < kMergeIpt; ++j) {
    const int p = i0 + j;
    if (p < m) f += (p == 0 || mk[p - 1] != mk[p]) ? 1 : 0;
  }
  int tot;
  const int ex = block_exclusive_scan(f, scan, &tot);
  if (threadIdx.x == 0) os_store(look + tile, kOsFlagA | (uint32_t)tot);
  {
    const uint32_t part = os_sum_before(look, tile, 1, threadIdx.x, kMergeThreads);
    int all;
    (void)block_exclusive_scan((int)part, scan, &all);
    if (threadIdx.x == 0) {
      prefix = all;
      n_heads = tot;
      if (tile == gridDim.x - 1) n_out[0] = all + tot;
    }
  }
  int o = ex;
#pragma unroll
  for (int j = 0; j < kMergeIpt; ++j) {
    const int p = i0 + j;
    if (p < m && (p == 0 || mk[p - 1] != mk[p])) hp[o++] = p;
  }
  __syncthreads();
  // per head: its one or two source rows, resolved once (LDS), uniq written
  for (int h = threadIdx.x; h < n_heads; h += kMergeThreads) {
    const int p = hp[h];
    const int32_t key = mk[p];
    const int r0 = ref[p];
    const bool two = p + 1 < m && mk[p + 1] == key;
    h0[h] = r0;                                    // A row, or B row | 0x80000000
    h1[h] = two ? (ref[p + 1] & 0x7fffffff) : -1;  // the B row of a row in both
    uniq_out[prefix + h] = key;
  }
  __syncthreads();
  // (head, column group) items over the block's lanes, eight items' loads in flight
  const int dv = d / V;
  const int items = n_heads * dv;
  for (int it0 = threadIdx.x; it0 < items; it0 += 8 * kMergeThreads) {
    float a[8][V], b[8][V];
    int hh[8], cc[8];
    bool tw[8], pre[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int it = min(it0 + j * kMergeThreads, items - 1);
      const int h = it / dv;
      cc[j] = (it - h * dv) * V;
      hh[j] = h;
      const int r0 = h0[h], r1 = h1[h];
      tw[j] = r1 >= 0;
      const bool fromA = r0 >= 0;
      pre[j] = fromA && a_pre;
      const float* s0 = (fromA ? rowsA + (int64_t)r0 * d
                               : rowsB + (int64_t)(r0 & 0x7fffffff) * d) + cc[j];
      const float* s1 = rowsB + (int64_t)(tw[j] ? r1 : 0) * d + cc[j];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        a[j][e] = s0[e];
        b[j][e] = s1[e];
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (it0 + j * kMergeThreads >= items) continue;
      merge_fold<V>(a[j], b[j], pre[j], tw[j], rows_out + (int64_t)(prefix + hh[j]) * d + cc[j]);
    }
  }
  os_cleanup(ticket, look, gridDim.x, &last);
}

// The scatter workspace: head [chunks][d] | tail [chunks][d] | (a pair's one-column
// head1 [chunks] | tail1 [chunks]) | tail_seg [chunks], chunks of scat_chunk(d) positions.
struct ScatWs {
  int chunks;
  float *head, *tail, *head1 = nullptr, *tail1 = nullptr;
  int32_t* tail_seg;
  ScatWs(void* ws, int64_t n, int d, bool pair)
      : chunks((int)((n + scat_chunk(d) - 1) / scat_chunk(d))) {
    head = (float*)ws;
    tail = head + (int64_t)chunks * d;
    float* end = tail + (int64_t)chunks * d;
    if (pair) {
      head1 = end;
      tail1 = head1 + chunks;
      end = tail1 + chunks;
    }
    tail_seg = (int32_t*)end;
  }
};

// the multi-piece segments' sums (a pair's one-column output: dense1), after any of the
// chunk kernels
static void launch_fixup(const ScatWs& W, int d, const int32_t* uniq, const int32_t* seg,
                         float* dense, int64_t n_rows, int compact, float* dense1,
                         hipStream_t st) {
  if (W.chunks > 1)
    hipLaunchKernelGGL(scatter_fixup_kernel,
                       dim3((unsigned)((W.chunks - 1 + kFixWaves - 1) / kFixWaves)),
                       dim3(64 * kFixWaves), 0, st, d, uniq, seg, W.tail_seg, dense, n_rows,
                       W.head, W.tail, W.chunks, compact, dense1, W.head1, W.tail1);
}

}  // namespace mirec

using namespace mirec;

extern "C" size_t mirec_segment_scatter_add_workspace_size(int64_t n, int32_t d) {
  const int64_t chunks = (n + kScatChunkMin - 1) / kScatChunkMin;
  return (size_t)2 * (size_t)chunks * (size_t)(d > 0 ? d : 1) * sizeof(float) +
         (size_t)chunks * sizeof(int32_t) + 256;
}

static int scatter_impl(const float* rows, int32_t d, const int32_t* perm, const int32_t* uniq,
                        const int32_t* seg, const int32_t* n_uniq_dev, int64_t n, float* dense,
                        int64_t n_rows, void* ws, size_t ws_bytes, int compact, void* stream) {
  if (n == 0) return 0;
  if (!rows || !perm || !uniq || !seg || !n_uniq_dev || !dense || d <= 0 || d > 256 || n < 0 ||
      n > INT32_MAX) {
    set_error("mirec_segment_scatter_add_f32: bad arguments (1 <= d <= 256)");
    return -1;
  }
  if (!ws || ws_bytes < mirec_segment_scatter_add_workspace_size(n, d)) {
    set_error("mirec_segment_scatter_add_f32: workspace too small");
    return -1;
  }
  const ScatWs W(ws, n, d, false);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_SCAT(GG, DM)                                                                     \
  {                                                                                           \
    const int64_t groups_per_block = 4 * (64 / GG);                                           \
    hipLaunchKernelGGL((scatter_chunks_kernel<GG, DM>),                                        \
                       dim3((unsigned)((W.chunks + groups_per_block - 1) / groups_per_block)), \
                       dim3(256), 0, st, rows, d, perm, uniq, seg, n_uniq_dev, dense, n_rows,  \
                       W.head, W.tail, W.tail_seg, W.chunks, compact);                         \
  }
  if (d == 1) MIREC_SCAT(1, 1)
  else if (d <= 4) MIREC_SCAT(4, 4)
  else if (d <= 16) MIREC_SCAT(16, 16)
  else if (d <= 32) MIREC_SCAT(32, 32)
  else if (d <= 64) MIREC_SCAT(64, 64)
  else MIREC_SCAT(64, 256)
#undef MIREC_SCAT
  launch_fixup(W, d, uniq, seg, dense, n_rows, compact, nullptr, st);
  return launch_status("mirec_segment_scatter_add_f32");
}

extern "C" int mirec_segment_scatter_add_f32(const float* rows, int32_t d, const int32_t* perm,
                                             const int32_t* uniq, const int32_t* seg,
                                             const int32_t* n_uniq_dev, int64_t n, float* dense,
                                             int64_t n_rows, void* ws, size_t ws_bytes,
                                             void* stream) {
  return scatter_impl(rows, d, perm, uniq, seg, n_uniq_dev, n, dense, n_rows, ws, ws_bytes, 0,
                      stream);
}

extern "C" int mirec_segment_reduce_f32(const float* rows, int32_t d, const int32_t* perm,
                                        const int32_t* uniq, const int32_t* seg,
                                        const int32_t* n_uniq_dev, int64_t n, float* out,
                                        void* ws, size_t ws_bytes, void* stream) {
  return scatter_impl(rows, d, perm, uniq, seg, n_uniq_dev, n, out, n, ws, ws_bytes, 1, stream);
}

static int reduce2_impl(const float* rows, int32_t d, const float* rows1, const int32_t* perm,
                        const int32_t* pos_seg, const int32_t* uniq, const int32_t* seg,
                        const int32_t* n_uniq_dev, int64_t n, float* out, float* out1, void* ws,
                        size_t ws_bytes, void* stream) {
  if (n == 0) return 0;
  if (!rows || !rows1 || !perm || !uniq || !seg || !n_uniq_dev || !out || !out1 || d < 2 ||
      d > 16 || n < 0 || n > INT32_MAX) {
    set_error("mirec_segment_reduce2_f32: bad arguments (2 <= d <= 16)");
    return -1;
  }
  if (!ws || ws_bytes < mirec_segment_scatter_add_workspace_size(n, d + 1)) {
    set_error("mirec_segment_reduce2_f32: workspace too small");
    return -1;
  }
  static_assert(MIREC_SCAT_NARROW_CH == 8, "the pair needs the one-column chunk size");
  const ScatWs W(ws, n, d, true);
  hipStream_t st = (hipStream_t)stream;
  const int64_t gpb = 4 * (64 / 16);
  if (pos_seg)
    hipLaunchKernelGGL((scatter_window_kernel<true>),
                       dim3((unsigned)((W.chunks + gpb - 1) / gpb)), dim3(256), 0, st, rows, d,
                       perm, pos_seg, uniq, seg, n_uniq_dev, out, n, W.head, W.tail, W.tail_seg,
                       W.chunks, 1, rows1, out1, W.head1, W.tail1);
  else if (d <= 4)
    hipLaunchKernelGGL((scatter_chunks_kernel<4, 4, true>),
                       dim3((unsigned)((W.chunks + 4 * 16 - 1) / (4 * 16))), dim3(256), 0, st,
                       rows, d, perm, uniq, seg, n_uniq_dev, out, n, W.head, W.tail, W.tail_seg,
                       W.chunks, 1, rows1, out1, W.head1, W.tail1);
  else
    hipLaunchKernelGGL((scatter_chunks_kernel<16, 16, true>),
                       dim3((unsigned)((W.chunks + gpb - 1) / gpb)), dim3(256), 0, st, rows, d,
                       perm, uniq, seg, n_uniq_dev, out, n, W.head, W.tail, W.tail_seg, W.chunks,
                       1, rows1, out1, W.head1, W.tail1);
  launch_fixup(W, d, uniq, seg, out, n, 1, out1, st);
  return launch_status("mirec_segment_reduce2_f32");
}

extern "C" int mirec_segment_reduce2_f32(const float* rows, int32_t d, const float* rows1,
                                         const int32_t* perm, const int32_t* uniq,
                                         const int32_t* seg, const int32_t* n_uniq_dev, int64_t n,
                                         float* out, float* out1, void* ws, size_t ws_bytes,
                                         void* stream) {
  return reduce2_impl(rows, d, rows1, perm, nullptr, uniq, seg, n_uniq_dev, n, out, out1, ws,
                      ws_bytes, stream);
}

extern "C" int mirec_segment_reduce2_pos_seg_f32(const float* rows, int32_t d,
                                                 const float* rows1, const int32_t* perm,
                                                 const int32_t* pos_seg, const int32_t* uniq,
                                                 const int32_t* seg, const int32_t* n_uniq_dev,
                                                 int64_t n, float* out, float* out1, void* ws,
                                                 size_t ws_bytes, void* stream) {
  if (!pos_seg) {
    set_error("mirec_segment_reduce2_pos_seg_f32: pos_seg is null");
    return -1;
  }
  return reduce2_impl(rows, d, rows1, perm, pos_seg, uniq, seg, n_uniq_dev, n, out, out1, ws,
                      ws_bytes, stream);
}

extern "C" int mirec_segment_reduce_pos_seg_f32(const float* rows, int32_t d,
                                                const int32_t* perm, const int32_t* pos_seg,
                                                const int32_t* uniq, const int32_t* seg,
                                                const int32_t* n_uniq_dev, int64_t n, float* out,
                                                void* ws, size_t ws_bytes, void* stream) {
  if (n == 0) return 0;
  if (!rows || !perm || !pos_seg || !uniq || !seg || !n_uniq_dev || !out || d <= 0 ||
      d > 256 || n < 0 || n > INT32_MAX) {
    set_error("mirec_segment_reduce_pos_seg_f32: bad arguments (1 <= d <= 256)");
    return -1;
  }
  if (!ws || ws_bytes < mirec_segment_scatter_add_workspace_size(n, d)) {
    set_error("mirec_segment_reduce_pos_seg_f32: workspace too small");
    return -1;
  }
  const ScatWs W(ws, n, d, false);
  hipStream_t st = (hipStream_t)stream;
  if (d <= 16) {
    const int64_t gpb = 4 * (64 / 16);
    hipLaunchKernelGGL((scatter_window_kernel<false>),
                       dim3((unsigned)((W.chunks + gpb - 1) / gpb)), dim3(256), 0, st, rows, d,
                       perm, pos_seg, uniq, seg, n_uniq_dev, out, n, W.head, W.tail, W.tail_seg,
                       W.chunks, 1, nullptr, nullptr, nullptr, nullptr);
  } else {
#define MIREC_WIDE(MC)                                                                        \
  hipLaunchKernelGGL((scatter_wide_window_kernel<MC>),                                        \
                     dim3((unsigned)((W.chunks + 3) / 4)), /* four waves (chunks) a block */  \
                     dim3(256), 0, st, rows, d, perm, pos_seg, uniq, seg, n_uniq_dev, out, n, \
                     W.head, W.tail, W.tail_seg, W.chunks, 1)
    if (d <= 64) MIREC_WIDE(1);
    else if (d <= 128) MIREC_WIDE(2);
    else MIREC_WIDE(4);
#undef MIREC_WIDE
  }
  launch_fixup(W, d, uniq, seg, out, n, 1, nullptr, st);
  return launch_status("mirec_segment_reduce_pos_seg_f32");
}

extern "C" int mirec_segment_merge2_f32(const int32_t* uA, const int32_t* nA_dev, int64_t capA,
                                        const float* rowsA, const int32_t* uB,
                                        const int32_t* nB_dev, int64_t capB, const float* rowsB,
                                        int32_t d, int32_t a_pre, int32_t* uniq_out,
                                        int32_t* n_out_dev, float* rows_out, void* ws,
                                        size_t ws_bytes, int32_t* status, int64_t n_status,
                                        void* stream) {
  const int64_t cap = capA + capB;
  if (!uA || !nA_dev || !rowsA || !uB || !nB_dev || !rowsB || !uniq_out || !n_out_dev ||
      !rows_out || !status || capA < 0 || capB < 0 || cap <= 0 || cap >= (int64_t)kOsVal ||
      d <= 0 || d > 1024) {
    set_error("mirec_segment_merge2_f32: bad arguments");
    return -1;
  }
  const int64_t tiles = (cap + kMergeTile - 1) / kMergeTile;
  if (!ws || ws_bytes < (size_t)(2 * cap) * sizeof(int32_t) || n_status < tiles + 1) {
    set_error("mirec_segment_merge2_f32: workspace (%lld B) or status (%lld words) too small",
              (long long)(2 * cap * 4), (long long)(tiles + 1));
    return -1;
  }
  int32_t* mk = (int32_t*)ws;
  int32_t* ref = mk + cap;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(merge_place_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, st,
                     uA, nA_dev, (int)capA, uB, nB_dev, (int)capB, mk, ref);
  if (d % 4 == 0)
    hipLaunchKernelGGL(merge_compact_kernel<4>, dim3((unsigned)tiles), dim3(kMergeThreads), 0, st,
                       mk, ref, nA_dev, nB_dev, rowsA, rowsB, d, a_pre, uniq_out, n_out_dev,
                       rows_out, (uint32_t*)status, (uint32_t*)status + tiles);
  else
    hipLaunchKernelGGL(merge_compact_kernel<1>, dim3((unsigned)tiles), dim3(kMergeThreads), 0, st,
                       mk, ref, nA_dev, nB_dev, rowsA, rowsB, d, a_pre, uniq_out, n_out_dev,
                       rows_out, (uint32_t*)status, (uint32_t*)status + tiles);
  return launch_status("mirec_segment_merge2_f32");
}
