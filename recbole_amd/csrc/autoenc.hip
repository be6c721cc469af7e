// K15 — the autoencoder family's sparse user rows (MultiDAE / MultiVAE). A batch row is
// the SET S_b of a user's history items (a CSR slice, distinct and ascending), never a dense
// [B, n_items] rating row. include/mirec.h (K15) states the arithmetic; this header states
// how each kernel runs. All fp32, no atomics, one owner and a fixed order per sum.
//
// Restates, for one batch:
//   get_rating_matrix + F.normalize + F.dropout + encoder[0] (+ Tanh)   (multivae.py:54-69,
//     89-93; multidae.py:51-66, 78-82) and the weight gradient of that Linear        K15a/b
//   -(F.log_softmax(z, 1) * rating_matrix).sum(1) and its backward  (multivae.py:119)  K15c
//   the pad / history mask, topk and pos_idx of a full-sort evaluation batch
//     (trainer.py:328-353, evaluators.py:65-75) for a given score matrix               K15d
//
// K15a bag_fwd_kernel: one workgroup (4 waves) per batch row; thread t owns the float4
//   column t of the output (N / 4 <= 256 columns). The row's items are cut into units of
//   kBagSplit = 64: lane j of the unit's wave holds item j and its keep flag, a ballot gives
//   the kept items, and the wave gathers their Wt rows whole (16 B per lane, up to 4 float4
//   per lane for N = 1024), FOUR rows in flight, adding them item after item. A round is 4
//   units (one per wave); after each round the 4 partial sums go through LDS and thread t
//   adds them to its total in unit order: total = (((total + u0) + u1) + u2) + u3. So
//   y[b] = act(bias + c_b * total) is one fixed sum whatever the row length. The keep flag
//   is drop.h's draw of element e = b * n_items + item.
// K15b bag_expand_kernel: one wave per batch row writes the row's (item, b, weight)
//   triples at off[b]..; the draw is the forward's (same key, same element index).
//   bag_bwd_chunk_kernel: one wave per kBagChunk = 32 sorted positions (K2's chunk). Lane j
//   reads position j's (item, b, weight) through perm; the wave walks the positions in
//   order, four G rows in flight, and closes a sum whenever the item changes. A run that
//   lies inside the chunk is stored to dWt[item]; a run that continues from the previous
//   chunk goes to the chunk's HEAD partial, one that starts here and continues into the next
//   chunk to its TAIL partial (a chunk has at most one of each; flags say which exist).
//   bag_bwd_fix_kernel: the wave of a chunk with a TAIL adds the following chunks' HEADs in
//   chunk order and stores dWt[item]. Positions inside a segment ascend in b (stable sort),
//   so every row of dWt is sum_b ascending. bag_bwd_zero_kernel: one wave per item; an item
//   that no sorted position holds (binary search through perm) gets a zero row.
// K15c nll_fwd_kernel / nll_bwd_kernel: one workgroup per row of z. The row's 16-B aligned
//   body moves as float4, the edges as scalars. Forward: per thread an online (max, sum)
//   with one rescale per float4, merged over the wave by an xor butterfly and over the 4
//   waves in wave order; then sum_{i in S_b} (lse - z[b, i]), thread-strided, reduced the
//   same way; the row's (max, sum) are kept for the backward. Backward: the dense pass
//   writes n_b exp(z - max) / sum * g / B, a barrier, then the
//   row's own workgroup subtracts g / B at the set's columns (distinct items: plain stores).
// K15d matrix_topk_kernel<KC>: one workgroup per query. Thread t scans items t, t + 256, ..
//   (increasing id, strict '>' insert, topk.h) into a KC-entry register list; an item is
//   looked up in the history only once it beats the list's last entry. Then K selection
//   rounds: the best list head by the full (score desc, id asc) order over the wave (xor
//   butterfly) and the 4 waves (LDS) is output, and the thread that owns it pops its list.
//   The matrix is given, so the ranking is exact.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): VGPRs / LDS bytes;
// no AGPRs, no scratch and no VGPR spills in any kernel.
//   float4 per lane (N <=)        1 (256)      2 (512)      3 (768)      4 (1024)
//   bag_fwd_kernel (either DROP)  34 / 16384   56 / 16384   74 / 16384   94 / 16384
//   bag_bwd_chunk_kernel          50 / 0       70 / 0       90 / 0       108 / 0
//   bag_bwd_fix_kernel            20 / 0       22 / 0       26 / 0       30 / 0
//   bag_expand_kernel 28 (19 without the draw) / 0      bag_bwd_zero_kernel 22 / 0
//   nll_fwd_kernel 24 / 32        nll_bwd_kernel 45 / 16
//   matrix_topk_kernel<10 / 20 / 50>  38 / 58 / 119 VGPRs, 32 B of LDS (K <= 50 moves 40
//   SGPRs into VGPR lanes)
#include "common.h"
#include "drop.h"
#include "topk.h"

namespace mirec {

constexpr int kBagThreads = 256;
constexpr int kBagSplit = MIREC_BAG_ROW_SPLIT;
constexpr int kBagChunk = MIREC_BAG_SEG_CHUNK;
static_assert(kBagSplit == 64, "a unit is one item per lane");
static_assert(kBagChunk <= 62, "a chunk is one position per lane; lanes 62 / 63 fetch its edges");

__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
  return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ float4 f4fma(float s, float4 a, float4 b) {
  return make_float4(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w));
}

__device__ __forceinline__ int uniform_lane_i(int v, int lane) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}

__device__ __forceinline__ float uniform_lane_f(float v, int lane) {
  return __int_as_float(uniform_lane_i(__float_as_int(v), lane));
}

// ------------------------------------------------------------------ K15a
// V: float4 per lane of a gathered row (N / 4 <= 64 V)
template <int V, bool DROP>
__global__ __launch_bounds__(kBagThreads) void bag_fwd_kernel(
    const int64_t* __restrict__ users, int64_t B, const int64_t* __restrict__ hptr,
    const int32_t* __restrict__ hcols, int64_t n_users, int64_t n_items,
    const float* __restrict__ Wt, const float* __restrict__ bias, int n4, uint32_t thr,
    float inv_keep, uint64_t seed, const int64_t* __restrict__ counter,
    int64_t* __restrict__ drawn, int act, float* __restrict__ y) {
  __shared__ float4 sP[4][kBagThreads];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x;
  const int64_t u = users[b];
  int64_t a = 0, e = 0;
  if (u >= 0 && u < n_users) { a = hptr[u]; e = hptr[u + 1]; }
  const int64_t nb = e > a ? e - a : 0;
  uint64_t key = 0;
  if (DROP) {
    const int64_t cv = counter[0];
    key = drop_key(seed, cv);
    if (b == 0 && tid == 0) drawn[0] = cv;
  }
  const float4* __restrict__ W4 = reinterpret_cast<const float4*>(Wt);
  float4 total = make_float4(0.f, 0.f, 0.f, 0.f);

  for (int64_t r0 = 0; r0 < nb; r0 += 4 * kBagSplit) {
    const int64_t j = r0 + (int64_t)w * kBagSplit + lane;
    int item = -1;
    if (j < nb) item = hcols[a + j];
    bool ok = item >= 0 && (int64_t)item < n_items;
    if (DROP && ok) ok = drop_keep(key, (uint64_t)b * (uint64_t)n_items + (uint64_t)item, thr);
    unsigned long long mask = __ballot(ok);
    float4 acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    while (mask) {
      int it[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        it[k] = -1;
        if (mask) {
          const int l = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          it[k] = uniform_lane_i(item, l);
        }
      }
      float4 rw[4][V];
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const int c = lane + 64 * v;
          rw[k][v] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (it[k] >= 0 && c < n4) rw[k][v] = W4[(int64_t)it[k] * n4 + c];
        }
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (it[k] >= 0) {
#pragma unroll
          for (int v = 0; v < V; ++v) acc[v] = f4add(acc[v], rw[k][v]);
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int c = lane + 64 * v;
      if (c < n4) sP[w][c] = acc[v];
    }
    __syncthreads();
    if (tid < n4) {
      total = f4add(total, sP[0][tid]);
      total = f4add(total, sP[1][tid]);
      total = f4add(total, sP[2][tid]);
      total = f4add(total, sP[3][tid]);
    }
    __syncthreads();
  }

  if (tid < n4) {
    float cb = 0.f;
    if (nb > 0) cb = (1.0f / sqrtf((float)nb)) * (DROP ? inv_keep : 1.0f);
    const float4 bi = reinterpret_cast<const float4*>(bias)[tid];
    float4 o = f4fma(cb, total, bi);
    if (act == 1) o = make_float4(tanhf(o.x), tanhf(o.y), tanhf(o.z), tanhf(o.w));
    reinterpret_cast<float4*>(y)[b * n4 + tid] = o;
  }
}

// ------------------------------------------------------------------ K15b
template <bool DROP>
__global__ __launch_bounds__(kBagThreads) void bag_expand_kernel(
    const int64_t* __restrict__ users, int64_t B, const int64_t* __restrict__ hptr,
    const int32_t* __restrict__ hcols, int64_t n_users, int64_t n_items,
    const int64_t* __restrict__ off, int64_t nnz, uint32_t thr, float inv_keep, uint64_t seed,
    const int64_t* __restrict__ drawn, int64_t* __restrict__ counter,
    int64_t* __restrict__ keys, int32_t* __restrict__ row_of, float* __restrict__ wgt) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (kBagThreads / 64) + (threadIdx.x >> 6);
  uint64_t key = 0;
  if (DROP) {
    const int64_t cv = drawn[0];
    key = drop_key(seed, cv);
    if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] = cv + 1;      // the next draw
  }
  if (b >= B) return;
  const int64_t u = users[b];
  int64_t a = 0, e = 0;
  if (u >= 0 && u < n_users) { a = hptr[u]; e = hptr[u + 1]; }
  const int64_t nb = e > a ? e - a : 0;
  const int64_t q0 = off[b];
  const float cb = nb > 0 ? (1.0f / sqrtf((float)nb)) * (DROP ? inv_keep : 1.0f) : 0.f;
  for (int64_t j = lane; j < nb; j += 64) {
    const int64_t q = q0 + j;
    if (q < 0 || q >= nnz) continue;                 // off disagrees with the CSR: write nothing
    const int item = hcols[a + j];
    bool ok = item >= 0 && (int64_t)item < n_items;
    if (DROP && ok) ok = drop_keep(key, (uint64_t)b * (uint64_t)n_items + (uint64_t)item, thr);
    keys[q] = item >= 0 && (int64_t)item < n_items ? (int64_t)item : 0;
    row_of[q] = (int32_t)b;
    wgt[q] = ok ? cb : 0.f;
  }
}

constexpr int kBagHead = 1, kBagTail = 2, kBagHeadOn = 4;   // flags of a chunk

// part [n_chunks][2][N]: HEAD then TAIL partial; flags / tail_item [n_chunks]
template <int V>
__global__ __launch_bounds__(kBagThreads) void bag_bwd_chunk_kernel(
    const float* __restrict__ G, int64_t B, int n4, int64_t nnz,
    const int64_t* __restrict__ keys, const int32_t* __restrict__ row_of,
    const float* __restrict__ wgt, const int32_t* __restrict__ perm, int64_t n_items,
    float* __restrict__ dWt, float* __restrict__ part, int32_t* __restrict__ flags,
    int32_t* __restrict__ tail_item) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kBagThreads / 64) + (threadIdx.x >> 6);
  const int64_t p0 = c * kBagChunk;
  if (p0 >= nnz) return;
  const int cnt = (int)(nnz - p0 < kBagChunk ? nnz - p0 : kBagChunk);
  // lane j: position p0 + j; lanes cnt and 63 fetch the item after and before the chunk
  int item = -1, brow = 0;
  float wt = 0.f;
  auto item_at = [&](int64_t p) -> int {
    const int q = perm[p];
    return (q >= 0 && (int64_t)q < nnz) ? (int)keys[q] : -1;
  };
  if (lane < cnt) {
    const int q = perm[p0 + lane];
    if (q >= 0 && (int64_t)q < nnz) {
      item = (int)keys[q];
      brow = row_of[q];
      wt = wgt[q];
      if (brow < 0 || (int64_t)brow >= B) wt = 0.f;
      if (item < 0 || (int64_t)item >= n_items) {
        item = -1;
        wt = 0.f;
      }
    }
  }
  int edge = -2;                                       // -2: no such position
  if (lane == 62 && p0 > 0) edge = item_at(p0 - 1);
  if (lane == 63 && p0 + cnt < nnz) edge = item_at(p0 + cnt);
  const int prev_item = uniform_lane_i(edge, 62);
  const int next_item = uniform_lane_i(edge, 63);

  const float4* __restrict__ G4 = reinterpret_cast<const float4*>(G);
  float4* __restrict__ D4 = reinterpret_cast<float4*>(dWt);
  float4* __restrict__ P4 = reinterpret_cast<float4*>(part) + c * 2 * n4;
  float4 acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  int cur = uniform_lane_i(item, 0), start = 0, fl = 0, titem = -1;

  // close the run [start, end) of item `cur`
  auto flush = [&](int end) {
    const bool head = start == 0 && prev_item == cur;
    const bool on = end == cnt && next_item == cur;
    float4* dst = nullptr;
    if (head) {
      dst = P4;
      fl |= kBagHead | (on ? kBagHeadOn : 0);
    } else if (on) {
      dst = P4 + n4;
      fl |= kBagTail;
      titem = cur;
    } else if (cur >= 0) {
      dst = D4 + (int64_t)cur * n4;
    }
    if (dst) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int col = lane + 64 * v;
        if (col < n4) dst[col] = acc[v];
      }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  };

  for (int j0 = 0; j0 < cnt; j0 += 4) {
    int itj[4], bj[4];
    float wj[4];
    float4 rw[4][V];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      itj[k] = -2;
      bj[k] = 0;
      wj[k] = 0.f;
      if (j < cnt) {
        itj[k] = uniform_lane_i(item, j);
        bj[k] = uniform_lane_i(brow, j);
        wj[k] = uniform_lane_f(wt, j);
      }
#pragma unroll
      for (int v = 0; v < V; ++v) {
        const int col = lane + 64 * v;
        rw[k][v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (wj[k] != 0.f && col < n4) rw[k][v] = G4[(int64_t)bj[k] * n4 + col];
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int j = j0 + k;
      if (j < cnt) {
        if (itj[k] != cur) {
          flush(j);
          cur = itj[k];
          start = j;
        }
        if (wj[k] != 0.f) {
#pragma unroll
          for (int v = 0; v < V; ++v) acc[v] = f4fma(wj[k], rw[k][v], acc[v]);
        }
      }
    }
  }
  flush(cnt);
  if (lane == 0) {
    flags[c] = fl;
    tail_item[c] = titem;
  }
}

template <int V>
__global__ __launch_bounds__(kBagThreads) void bag_bwd_fix_kernel(
    int n4, int64_t n_chunks, int64_t n_items, float* __restrict__ dWt,
    const float* __restrict__ part, const int32_t* __restrict__ flags,
    const int32_t* __restrict__ tail_item) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kBagThreads / 64) + (threadIdx.x >> 6);
  if (c >= n_chunks || !(flags[c] & kBagTail)) return;
  const int item = tail_item[c];
  if (item < 0 || (int64_t)item >= n_items) return;
  const float4* __restrict__ P4 = reinterpret_cast<const float4*>(part);
  float4 acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int col = lane + 64 * v;
    acc[v] = col < n4 ? P4[(c * 2 + 1) * n4 + col] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  for (int64_t cc = c + 1; cc < n_chunks; ++cc) {
    const int f = flags[cc];
    if (!(f & kBagHead)) break;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const int col = lane + 64 * v;
      if (col < n4) acc[v] = f4add(acc[v], P4[cc * 2 * n4 + col]);
    }
    if (!(f & kBagHeadOn)) break;
  }
  float4* __restrict__ D4 = reinterpret_cast<float4*>(dWt) + (int64_t)item * n4;
#pragma unroll
  for (int v = 0; v < V; ++v) {
    const int col = lane + 64 * v;
    if (col < n4) D4[col] = acc[v];
  }
}

__global__ __launch_bounds__(kBagThreads) void bag_bwd_zero_kernel(
    int n4, int64_t nnz, const int64_t* __restrict__ keys, const int32_t* __restrict__ perm,
    int64_t n_items, float* __restrict__ dWt) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (kBagThreads / 64) + (threadIdx.x >> 6);
  if (i >= n_items) return;
  int64_t lo = 0, hi = nnz;                           // first sorted position with item >= i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int q = perm[mid];
    const int64_t k = (q >= 0 && (int64_t)q < nnz) ? keys[q] : INT64_MAX;
    if (k < i) lo = mid + 1; else hi = mid;
  }
  bool present = false;
  if (lo < nnz) {
    const int q = perm[lo];
    present = q >= 0 && (int64_t)q < nnz && keys[q] == i;
  }
  if (present) return;
  float4* __restrict__ D4 = reinterpret_cast<float4*>(dWt) + i * n4;
  for (int col = lane; col < n4; col += 64) D4[col] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------ K15c
constexpr int kNllThreads = 256;

__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  if (mm == -INFINITY) { m = mm; s = 0.f; return; }
  s = s * expf(m - mm) + s2 * expf(m2 - mm);
  m = mm;
}

__device__ __forceinline__ void ms_add4(float& m, float& s, float4 x) {
  const float m4 = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
  if (m4 > m) {
    s *= expf(m - m4);                                // m = -inf: s is 0 and stays 0
    m = m4;
  }
  if (m == -INFINITY) return;
  s += (expf(x.x - m) + expf(x.y - m)) + (expf(x.z - m) + expf(x.w - m));
}

__device__ __forceinline__ void ms_add1(float& m, float& s, float x) {
  if (x > m) {
    s *= expf(m - x);
    m = x;
  }
  if (m == -INFINITY) return;
  s += expf(x - m);
}

// The row's split: [0, head) scalars, [head, head + 4 nv) float4, the rest scalars.
__device__ __forceinline__ void row_split(const float* row, int64_t I, int64_t* head,
                                          int64_t* nv) {
  const int64_t mis = (int64_t)(((uintptr_t)row >> 2) & 3);     // floats past a 16-B boundary
  int64_t h = (4 - mis) & 3;
  if (((uintptr_t)row & 3) || h > I) { *head = I; *nv = 0; return; }
  *head = h;
  *nv = (I - h) >> 2;
}

__global__ __launch_bounds__(kNllThreads) void nll_fwd_kernel(
    const float* __restrict__ z, int64_t ld, int64_t I, const int64_t* __restrict__ users,
    const int64_t* __restrict__ hptr, const int32_t* __restrict__ hcols, int64_t n_users,
    float* __restrict__ lse, float* __restrict__ stat, float* __restrict__ loss_rows) {
  __shared__ float sm[4], ss[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t b = blockIdx.x;
  const float* __restrict__ row = z + b * ld;
  int64_t head, nv;
  row_split(row, I, &head, &nv);
  float m = -INFINITY, s = 0.f;
  for (int64_t i = tid; i < head; i += kNllThreads) ms_add1(m, s, row[i]);
  const float4* __restrict__ r4 = reinterpret_cast<const float4*>(row + head);
  for (int64_t i = tid; i < nv; i += kNllThreads) ms_add4(m, s, r4[i]);
  for (int64_t i = head + 4 * nv + tid; i < I; i += kNllThreads) ms_add1(m, s, row[i]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
    ms_merge(m, s, m2, s2);
  }
  if (lane == 0) { sm[w] = m; ss[w] = s; }
  __syncthreads();
  m = sm[0];
  s = ss[0];
  for (int k = 1; k < 4; ++k) ms_merge(m, s, sm[k], ss[k]);
  const float l = m + logf(s);
  __syncthreads();                                      // sm / ss are reused below

  const int64_t u = users[b];
  int64_t a = 0, e = 0;
  if (u >= 0 && u < n_users) { a = hptr[u]; e = hptr[u + 1]; }
  float acc = 0.f;
  for (int64_t j = a + tid; j < e; j += kNllThreads) {
    const int item = hcols[j];
    if (item >= 0 && (int64_t)item < I) acc += l - row[item];
  }
  acc = wave_sum(acc);
  if (lane == 0) ss[w] = acc;
  __syncthreads();
  if (tid == 0) {
    lse[b] = l;
    stat[2 * b] = m;
    stat[2 * b + 1] = s;
    loss_rows[b] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
  }
}

__global__ __launch_bounds__(kNllThreads) void nll_bwd_kernel(
    float* __restrict__ z, int64_t ld, int64_t B, int64_t I, const int64_t* __restrict__ users,
    const int64_t* __restrict__ hptr, const int32_t* __restrict__ hcols, int64_t n_users,
    const float* __restrict__ stat, const float* __restrict__ g) {
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  float* __restrict__ row = z + b * ld;
  const int64_t u = users[b];
  int64_t a = 0, e = 0;
  if (u >= 0 && u < n_users) { a = hptr[u]; e = hptr[u + 1]; }
  // n_b counts the items the forward counted
  int nbl = 0;
  for (int64_t j = a + tid; j < e; j += kNllThreads) {
    const int item = hcols[j];
    nbl += (item >= 0 && (int64_t)item < I) ? 1 : 0;
  }
  __shared__ int sn[4];
  nbl = wave_sum_i(nbl);
  if ((tid & 63) == 0) sn[tid >> 6] = nbl;
  __syncthreads();
  const float nb = (float)(sn[0] + sn[1] + sn[2] + sn[3]);
  const float scale = g[0] / (float)B;
  // softmax = exp(z - max) / sum from the forward's (max, sum): z - max is exact near the
  // maximum, where log-sum-exp rounded to fp32 at |lse| ~ 80 would cost 4e-6 of every term
  const float l = stat[2 * b];
  const float ns = nb * scale / stat[2 * b + 1];
  int64_t head, nv;
  row_split(row, I, &head, &nv);
  for (int64_t i = tid; i < head; i += kNllThreads) row[i] = ns * expf(row[i] - l);
  float4* __restrict__ r4 = reinterpret_cast<float4*>(row + head);
  for (int64_t i = tid; i < nv; i += kNllThreads) {
    const float4 x = r4[i];
    r4[i] = make_float4(ns * expf(x.x - l), ns * expf(x.y - l), ns * expf(x.z - l),
                        ns * expf(x.w - l));
  }
  for (int64_t i = head + 4 * nv + tid; i < I; i += kNllThreads)
    row[i] = ns * expf(row[i] - l);
  __syncthreads();                        // the dense pass's stores are visible to the workgroup
  for (int64_t j = a + tid; j < e; j += kNllThreads) {
    const int item = hcols[j];
    if (item >= 0 && (int64_t)item < I) row[item] -= scale;
  }
}

// ------------------------------------------------------------------ K15d
constexpr int kMtThreads = 256;

template <int KC>
__global__ __launch_bounds__(kMtThreads) void matrix_topk_kernel(
    const float* __restrict__ S, int64_t I, int64_t ld, const int64_t* __restrict__ hist_ptr,
    const int32_t* __restrict__ hist_cols, const int64_t* __restrict__ pos_ptr,
    const int32_t* __restrict__ pos_cols, int K, float* __restrict__ top_scores,
    int32_t* __restrict__ top_ids, uint8_t* __restrict__ pos_flags) {
  __shared__ float sS[4];
  __shared__ int sI[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t q = blockIdx.x;
  const float* __restrict__ row = S + q * ld;
  const int64_t h0 = hist_ptr ? hist_ptr[q] : 0, h1 = hist_ptr ? hist_ptr[q + 1] : 0;
  float ts[KC];
  int ti[KC];
#pragma unroll
  for (int t = 0; t < KC; ++t) { ts[t] = -INFINITY; ti[t] = -1; }
  float thr = -INFINITY;
  for (int64_t i = tid; i < I; i += kMtThreads) {
    const float v = row[i];
    if (v > thr && i != 0 && !sorted_contains(hist_cols, h0, h1, (int32_t)i)) {
      topk_insert<KC>(ts, ti, v, (int)i);
      thr = ts[KC - 1];
    }
  }
  // K selection rounds over the 256 sorted lists: the best head by (score desc, id asc)
  // over the wave (xor butterfly) and over the 4 waves (LDS), thread 0 stores it, and the
  // one thread that owns it (an item is scanned by exactly one thread) pops its list.
  const int64_t p0 = pos_ptr ? pos_ptr[q] : 0, p1 = pos_ptr ? pos_ptr[q + 1] : 0;
  for (int r = 0; r < K; ++r) {
    float v = ts[0];
    int id = ti[0] < 0 ? INT32_MAX : ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oid = __shfl_xor(id, o, 64);
      const bool better = (ov > v) | ((ov == v) & (oid < id));
      v = better ? ov : v;
      id = better ? oid : id;
    }
    if (lane == 0) { sS[w] = v; sI[w] = id; }
    __syncthreads();
    v = sS[0];
    id = sI[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
      const float ov = sS[k];
      const int oid = sI[k];
      const bool better = (ov > v) | ((ov == v) & (oid < id));
      v = better ? ov : v;
      id = better ? oid : id;
    }
    __syncthreads();                                     // sS / sI are rewritten next round
    const bool none = id == INT32_MAX;
    if (tid == 0) {
      const int64_t o = q * K + r;
      if (top_scores) top_scores[o] = none ? -INFINITY : v;
      if (top_ids) top_ids[o] = none ? -1 : id;
      if (pos_flags) pos_flags[o] = (!none && sorted_contains(pos_cols, p0, p1, id)) ? 1 : 0;
    }
    const bool mine = !none & (ti[0] == id);
#pragma unroll
    for (int t = 0; t < KC - 1; ++t) {
      ts[t] = mine ? ts[t + 1] : ts[t];
      ti[t] = mine ? ti[t + 1] : ti[t];
    }
    ts[KC - 1] = mine ? -INFINITY : ts[KC - 1];
    ti[KC - 1] = mine ? -1 : ti[KC - 1];
  }
}

static bool bag_width_ok(int32_t N) { return N >= 4 && N <= 1024 && N % 4 == 0; }

}  // namespace mirec

using namespace mirec;

#define MIREC_BAG_V(n4, CALL)                 \
  do {                                        \
    if ((n4) <= 64) { CALL(1); }              \
    else if ((n4) <= 128) { CALL(2); }        \
    else if ((n4) <= 192) { CALL(3); }        \
    else { CALL(4); }                         \
  } while (0)

extern "C" int mirec_bag_linear_fwd_f32(const int64_t* users, int64_t B, const int64_t* hist_ptr,
                                        const int32_t* hist_cols, int64_t n_users,
                                        int64_t n_items, const float* Wt, const float* bias,
                                        int32_t N, float p, uint64_t seed,
                                        const int64_t* counter, int64_t* drawn, int32_t train,
                                        int32_t act, float* y, void* stream) {
  if (B == 0) return 0;
  const bool drop = train != 0 && p > 0.f;
  if (!users || !hist_ptr || !hist_cols || !Wt || !bias || !y || B < 0 || B > INT32_MAX ||
      n_users <= 0 || n_items <= 0 || n_items > INT32_MAX || !bag_width_ok(N) ||
      (act != 0 && act != 1) || ((uintptr_t)Wt % 16) || ((uintptr_t)bias % 16) ||
      ((uintptr_t)y % 16) || (drop && (!(p < 1.f) || !counter || !drawn))) {
    set_error("mirec_bag_linear_fwd_f32: bad arguments (N a multiple of 4 in 4..1024, 16-B "
              "aligned Wt / bias / y, act 0 or 1, training dropout needs 0 < p < 1 with the "
              "counter and the drawn word)");
    return -1;
  }
  const int n4 = N / 4;
  const uint32_t thr = drop ? drop_threshold(p) : 0u;
  const float inv_keep = drop ? 1.0f / (1.0f - p) : 1.0f;
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CALL(VV)                                                                          \
  if (drop)                                                                                     \
    hipLaunchKernelGGL((bag_fwd_kernel<VV, true>), dim3((unsigned)B), dim3(kBagThreads), 0, st, \
                       users, B, hist_ptr, hist_cols, n_users, n_items, Wt, bias, n4, thr,      \
                       inv_keep, seed, counter, drawn, (int)act, y);                            \
  else                                                                                          \
    hipLaunchKernelGGL((bag_fwd_kernel<VV, false>), dim3((unsigned)B), dim3(kBagThreads), 0,    \
                       st, users, B, hist_ptr, hist_cols, n_users, n_items, Wt, bias, n4, thr,  \
                       inv_keep, seed, counter, drawn, (int)act, y)
  MIREC_BAG_V(n4, MIREC_CALL);
#undef MIREC_CALL
  return launch_status("mirec_bag_linear_fwd_f32");
}

extern "C" int mirec_bag_expand_f32(const int64_t* users, int64_t B, const int64_t* hist_ptr,
                                    const int32_t* hist_cols, int64_t n_users, int64_t n_items,
                                    const int64_t* off, int64_t nnz, float p, uint64_t seed,
                                    const int64_t* drawn, int64_t* counter, int32_t train,
                                    int64_t* keys, int32_t* row_of, float* wgt, void* stream) {
  if (B == 0) return 0;
  const bool drop = train != 0 && p > 0.f;
  if (!users || !hist_ptr || !hist_cols || !off || B < 0 || B > INT32_MAX || n_users <= 0 ||
      n_items <= 0 || n_items > INT32_MAX || nnz < 0 || nnz > INT32_MAX ||
      (nnz > 0 && (!keys || !row_of || !wgt)) ||
      (drop && (!(p < 1.f) || !counter || !drawn))) {
    set_error("mirec_bag_expand_f32: bad arguments (nnz <= 2^31 - 1, training dropout needs "
              "0 < p < 1 with the counter and the drawn word)");
    return -1;
  }
  const uint32_t thr = drop ? drop_threshold(p) : 0u;
  const float inv_keep = drop ? 1.0f / (1.0f - p) : 1.0f;
  const int rpb = kBagThreads / 64;
  const dim3 grid((unsigned)((B + rpb - 1) / rpb));
  hipStream_t st = (hipStream_t)stream;
  if (drop)
    hipLaunchKernelGGL(bag_expand_kernel<true>, grid, dim3(kBagThreads), 0, st, users, B,
                       hist_ptr, hist_cols, n_users, n_items, off, nnz, thr, inv_keep, seed,
                       drawn, counter, keys, row_of, wgt);
  else
    hipLaunchKernelGGL(bag_expand_kernel<false>, grid, dim3(kBagThreads), 0, st, users, B,
                       hist_ptr, hist_cols, n_users, n_items, off, nnz, thr, inv_keep, seed,
                       drawn, counter, keys, row_of, wgt);
  return launch_status("mirec_bag_expand_f32");
}

static int64_t bag_chunks(int64_t nnz) { return (nnz + kBagChunk - 1) / kBagChunk; }

// part floats, then flags and tail items
extern "C" size_t mirec_bag_linear_bwd_workspace_size(int64_t nnz, int32_t N) {
  if (nnz <= 0 || N <= 0) return 16;
  const int64_t nc = bag_chunks(nnz);
  return (size_t)nc * 2 * (size_t)N * sizeof(float) + (size_t)nc * 2 * sizeof(int32_t) + 16;
}

extern "C" int mirec_bag_linear_bwd_f32(const float* G, int64_t B, int32_t N, int64_t nnz,
                                        const int64_t* keys, const int32_t* row_of,
                                        const float* wgt, const int32_t* perm, int64_t n_items,
                                        float* dWt, void* ws, size_t ws_bytes, void* stream) {
  if (!dWt || n_items <= 0 || n_items > INT32_MAX || !bag_width_ok(N) || nnz < 0 ||
      nnz > INT32_MAX || B < 0 || B > INT32_MAX || ((uintptr_t)dWt % 16) ||
      (nnz > 0 && (!G || !keys || !row_of || !wgt || !perm || !ws || ((uintptr_t)G % 16) ||
                   ((uintptr_t)ws % 16) ||
                   ws_bytes < mirec_bag_linear_bwd_workspace_size(nnz, N)))) {
    set_error("mirec_bag_linear_bwd_f32: bad arguments (N a multiple of 4 in 4..1024, 16-B "
              "aligned G / dWt / ws, ws of mirec_bag_linear_bwd_workspace_size bytes)");
    return -1;
  }
  const int n4 = N / 4;
  const int wpb = kBagThreads / 64;
  hipStream_t st = (hipStream_t)stream;
  if (nnz > 0) {
    const int64_t nc = bag_chunks(nnz);
    float* part = (float*)ws;
    int32_t* flags = (int32_t*)(part + (size_t)nc * 2 * N);
    int32_t* tail_item = flags + nc;
    const dim3 grid((unsigned)((nc + wpb - 1) / wpb));
#define MIREC_CALL(VV)                                                                        \
  hipLaunchKernelGGL(bag_bwd_chunk_kernel<VV>, grid, dim3(kBagThreads), 0, st, G, B, n4, nnz, \
                     keys, row_of, wgt, perm, n_items, dWt, part, flags, tail_item);          \
  hipLaunchKernelGGL(bag_bwd_fix_kernel<VV>, grid, dim3(kBagThreads), 0, st, n4, nc, n_items, \
                     dWt, part, flags, tail_item)
    MIREC_BAG_V(n4, MIREC_CALL);
#undef MIREC_CALL
    const int rc = launch_status("mirec_bag_linear_bwd_f32");
    if (rc) return rc;
  }
  hipLaunchKernelGGL(bag_bwd_zero_kernel, dim3((unsigned)((n_items + wpb - 1) / wpb)),
                     dim3(kBagThreads), 0, st, n4, nnz, keys, perm, n_items, dWt);
  return launch_status("mirec_bag_linear_bwd_f32");
}

static int nll_check(const void* z, int64_t ld, int64_t B, int64_t I, const void* users,
                     const void* hp, const void* hc, int64_t n_users, const void* lse,
                     const void* x, const char* what) {
  if (!z || !users || !hp || !hc || !lse || !x || B < 0 || B > INT32_MAX || I <= 0 ||
      I > INT32_MAX || ld < I || n_users <= 0 || ((uintptr_t)z % 4)) {
    set_error("%s: bad arguments (1 <= I <= 2^31 - 1, ld >= I)", what);
    return -1;
  }
  return 0;
}

extern "C" int mirec_multinomial_nll_fwd_f32(const float* z, int64_t ld, int64_t B, int64_t I,
                                             const int64_t* users, const int64_t* hist_ptr,
                                             const int32_t* hist_cols, int64_t n_users,
                                             float* lse, float* stat, float* loss_rows,
                                             void* stream) {
  if (B == 0) return 0;
  if (nll_check(z, ld, B, I, users, hist_ptr, hist_cols, n_users, lse, loss_rows,
                "mirec_multinomial_nll_fwd_f32"))
    return -1;
  if (!stat) {
    set_error("mirec_multinomial_nll_fwd_f32: stat is NULL");
    return -1;
  }
  hipLaunchKernelGGL(nll_fwd_kernel, dim3((unsigned)B), dim3(kNllThreads), 0,
                     (hipStream_t)stream, z, ld, I, users, hist_ptr, hist_cols, n_users, lse,
                     stat, loss_rows);
  return launch_status("mirec_multinomial_nll_fwd_f32");
}

extern "C" int mirec_multinomial_nll_bwd_f32(float* z, int64_t ld, int64_t B, int64_t I,
                                             const int64_t* users, const int64_t* hist_ptr,
                                             const int32_t* hist_cols, int64_t n_users,
                                             const float* stat, const float* g, void* stream) {
  if (B == 0) return 0;
  if (nll_check(z, ld, B, I, users, hist_ptr, hist_cols, n_users, stat, g,
                "mirec_multinomial_nll_bwd_f32"))
    return -1;
  hipLaunchKernelGGL(nll_bwd_kernel, dim3((unsigned)B), dim3(kNllThreads), 0,
                     (hipStream_t)stream, z, ld, B, I, users, hist_ptr, hist_cols, n_users, stat,
                     g);
  return launch_status("mirec_multinomial_nll_bwd_f32");
}

extern "C" int mirec_matrix_topk_f32(const float* scores, int64_t nq, int64_t I, int64_t ld,
                                     const int64_t* hist_ptr, const int32_t* hist_cols,
                                     const int64_t* pos_ptr, const int32_t* pos_cols, int32_t K,
                                     float* top_scores, int32_t* top_ids, uint8_t* pos_flags,
                                     void* stream) {
  if (nq == 0) return 0;
  if (!scores || nq < 0 || nq > INT32_MAX || I <= 0 || I > INT32_MAX || ld < I || K < 1 ||
      K > 50 || (hist_ptr && !hist_cols) || (pos_ptr && !pos_cols) || (pos_flags && !pos_ptr)) {
    set_error("mirec_matrix_topk_f32: bad arguments (1 <= K <= 50, I <= 2^31 - 1, ld >= I)");
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
#define MIREC_MT(KK)                                                                          \
  hipLaunchKernelGGL(matrix_topk_kernel<KK>, dim3((unsigned)nq), dim3(kMtThreads), 0, st,     \
                     scores, I, ld, hist_ptr, hist_cols, pos_ptr, pos_cols, (int)K, top_scores, \
                     top_ids, pos_flags)
  if (K <= 10) MIREC_MT(10);
  else if (K <= 20) MIREC_MT(20);
  else MIREC_MT(50);
#undef MIREC_MT
  return launch_status("mirec_matrix_topk_f32");
}
