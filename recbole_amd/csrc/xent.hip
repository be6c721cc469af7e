// K12 — full-catalogue cross entropy for the sequential models: the [B x n_items]
// logits are formed on FP32 MFMA tile by tile and consumed in registers, in the
// forward by an online log-sum-exp and in the backward by recomputation, so no
// B x n_items matrix (logits, log-softmax or its gradient) ever exists in HBM.
//
// Restates, for one batch:
//   SASRec.calculate_loss, loss_type 'CE'                       (sasrec.py:135-141)
//     logits = seq_output @ item_embedding.weight^T    (all rows, the padding row 0 too)
//     loss   = CrossEntropyLoss(logits, pos_items)     (mean over the batch)
//   and its autograd backward, with w[b,i] = (softmax(logits)[b,i] - [i == target[b]]) * g / B:
//     gS[b] = sum_i w[b,i] E[i]          dE[i] = sum_b w[b,i] S[b]
//
// Tiling (gfx950, wave64), K6's: a workgroup = 4 waves = 128 FIXED rows; each wave
// keeps its 32 fixed rows in registers as the MFMA B operand of
// v_mfma_f32_32x32x2_f32 and sweeps the OTHER matrix in tiles of 32 rows (one or two per
// staged tile, XeSub) staged once per workgroup in LDS, double buffered, rows
// padded to d + 2 floats. The k order of the dot product is K6's permuted one
// (k = 4*(s>>1) + 2h + (s&1)); all three kernels use the same order, so a logit
// recomputed in the backward is bit for bit the forward's.
//   K12a forward        fixed = queries, swept = items [ilo, ihi) of its item split
//   K12b backward, gS   fixed = queries, swept = items [ilo, ihi) of its item split
//   K12c backward, dE   fixed = items,   swept = ALL queries, ascending
// The 32x32 logits accumulator has the FIXED row on the lane column and 16 SWEPT
// rows per lane (rows (r&3) + 8*(r>>2) + 4h of the sub-tile).
//
// K12a: each lane keeps (max, sum, target logit) of its query over its 16 rows of every
// sub-tile: the sub-tile maximum first, one rescale of the running sum, then one exp per
// logit, added in register order r = 0..15. Items at or past the split's end count as
// -inf. The target logit is found by comparing the item id with target[q]; target never
// indexes memory, so a target outside [0, I) reads nothing (that row's loss is then +inf
// — unspecified). The two lane halves of a query merge at the end (half 0 first), each
// split writes its partial to the workspace, and xent_finish_kernel folds the partials
// in ascending split order: lse = max + log(sum), loss_rows = lse - target logit.
//
// K12b / K12c: the logits tile is recomputed, w formed in place, and the accumulator
// registers are then used AS THEY STAND as the A operand of the second product: register
// r of lane (j, h) is w[swept row (r&3) + 8*(r>>2) + 4h][fixed row j], which is A[i = j]
// [k = h] of a k-step over exactly those two swept rows, so w needs no LDS round trip. The B
// operand is the staged tile again (one ds_read_b32 per MFMA, lanes on consecutive
// columns). Each output element out[fixed row][column] is therefore one f32 fma chain
// over the swept rows in the order: tiles ascending, sub-tiles ascending, r = 0..15,
// h = 0 then 1. K12b with an item split writes partials [splits, B, d] summed by
// xent_sum_kernel in ascending split order; K12c has no split and stores every row of
// dE exactly once (the caller allocates with empty). No atomics anywhere.
//
// d = 256: the operand (128 VGPRs) plus the 32 x 256 output accumulator (128) do not fit
// two waves per SIMD; the kernels run ONE wave per SIMD there (a 512-register budget), in
// one pass.
//
// Resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), VGPRs (incl.
// AGPRs) / LDS bytes, no spills at any width:
//   d        32            64            128           256
//   K12a     103 / 17408   107 / 33792   191 / 66560   282 / 66048
//   K12b     116 / 17408   163 / 33792   238 / 33280   398 / 66048
//   K12c     127 / 18944   183 / 35328   232 / 34048   386 / 66816
// Over gathered rows (ROWS, K17: mirec_rows_ce_*), the same LDS, no spills:
//   K12a     103           107           191           282
//   K12b     115           162           236           411
//   K12c     126           182           231           384
#include "common.h"
#include "mfma.h"

namespace mirec {


constexpr int kXeThreads = 256;
constexpr int kXeFwd = 0, kXeQuery = 1, kXeItem = 2;
constexpr int64_t kXeTile = 64;       // a split's span is a multiple of every width's tile

// 32-row sub-tiles per staged tile: two while the registers allow (one barrier per 64
// swept rows); the backward at d = 128 stages 32 rows at a time — half the prefetch
// registers, and its sub-tile already carries 128 MFMAs per wave between barriers.
template <int D, int MODE> struct XeSub {
  static constexpr int n = (MODE == 0 ? D <= 128 : D <= 64) ? 2 : 1;
};

// X: the fixed matrix [NX, D] (queries S for K12a/b, items E for K12c); Y: the swept
// matrix [NY, D], this workgroup's rows [blockIdx.y * span, + span).
//   kXeFwd:   pm / ps / pt [gridDim.y, B] partial (max, sum, target logit or -inf)
//   kXeQuery: out [gridDim.y, B, D] partial gS (gS itself when gridDim.y == 1)
//   kXeItem:  out = dE [I, D]
// ROWS (K17, the queries are gathered rows of a larger matrix): query r is row rows[r] of the
// query matrix, loaded straight into the operand (K12a/b) or the staged tile (K12c); only
// queries r < min(count given to the launch, *n_dev) exist (n_dev null: all of them). A
// query workgroup that starts at or past that count leaves at once (K12b without a split
// writes its rows' zeros first), K12c's sweep ends there, and the backward's factor is
// g_dev[0] as it stands. Everything else — tiles, k order, summation orders — is the code
// below, shared.
template <int D, int MODE, bool ROWS>
__global__ __launch_bounds__(kXeThreads, D <= 128 ? 2 : 1) void xent_kernel(
    const float* __restrict__ X, int64_t NX, const float* __restrict__ Y, int64_t NY,
    const int64_t* __restrict__ target, const float* __restrict__ lse,
    const float* __restrict__ g_dev, int64_t B, int64_t span, float* __restrict__ out,
    float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ pt,
    const int64_t* __restrict__ rows, const int32_t* __restrict__ n_dev) {
  constexpr int LDR = D + 2;
  constexpr int V4 = D / 4;
  constexpr int NT = XeSub<D, MODE>::n;
  constexpr int TI = 32 * NT;
  constexpr int NPF = TI * V4 / kXeThreads;      // float4 per thread per tile (exact)
  static_assert(NPF * kXeThreads == TI * V4, "tile is a whole number of float4 rounds");
  constexpr int NM = MODE == kXeItem ? TI : 1;
  __shared__ __attribute__((aligned(16))) float tile[2][TI * LDR];
  __shared__ float s_lse[2][NM];         // K12c: lse / target of the staged queries
  __shared__ int64_t s_tgt[2][NM];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int j = lane & 31;
  const int h = lane >> 5;
  const int64_t xb = ((int64_t)blockIdx.x * 4 + w) * 32;
  const int64_t x = xb + j;
  const int64_t ylo = (int64_t)blockIdx.y * span;
  int64_t nx = NX, yhi = min(NY, ylo + span);
  if constexpr (ROWS) {
    const int64_t cnt = n_dev ? (int64_t)max(n_dev[0], 0) : INT64_MAX;
    if constexpr (MODE == kXeItem) {
      yhi = min(yhi, cnt);
    } else {
      nx = min(NX, cnt);
      const int64_t b0 = (int64_t)blockIdx.x * 128;
      if (b0 >= nx) {                      // no live query in this workgroup
        if (MODE == kXeQuery && gridDim.y == 1) {
          const int64_t n4 = (min(NX, b0 + 128) - b0) * (D / 4);
          float4* z = reinterpret_cast<float4*>(out + b0 * D);
          for (int64_t e = threadIdx.x; e < n4; e += kXeThreads)
            z[e] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
      }
    }
  }
  const bool xv = x < nx;
  int64_t xsrc = x;                        // the row of X this lane's fixed row is read from
  if constexpr (ROWS && MODE != kXeItem) xsrc = xv ? rows[x] : 0;

  // lane (j, h) holds fixed row x's elements in the permuted k order
  float ub[D / 2];
#pragma unroll
  for (int s2 = 0; s2 < D / 4; ++s2) {
    float2 v = make_float2(0.f, 0.f);
    if (xv) v = *reinterpret_cast<const float2*>(X + xsrc * D + 4 * s2 + 2 * h);
    ub[2 * s2] = v.x;
    ub[2 * s2 + 1] = v.y;
  }

  // per-lane state of the fixed row
  float m = -INFINITY, s = 0.f, tl = -INFINITY;               // K12a
  float lq = 0.f, scale = 0.f;
  int64_t tq = -1;
  if (MODE != kXeFwd) scale = ROWS ? g_dev[0] : g_dev[0] / (float)B;
  if (MODE != kXeItem && xv) tq = target[x];
  if (MODE == kXeQuery && xv) lq = lse[x];
  constexpr int NCB = MODE == kXeFwd ? 1 : D / 32;
  floatx16 oacc[NCB];
  if (MODE != kXeFwd) {
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[cb][r] = 0.f;
  }

  const float4* __restrict__ Y4 = reinterpret_cast<const float4*>(Y);
  float4 pf[NPF];
  auto load_tile = [&](int64_t base) {
#pragma unroll
    for (int k = 0; k < NPF; ++k) {
      const int f = threadIdx.x + k * kXeThreads;
      const int row = f / V4;
      const int c4 = f - row * V4;
      const int64_t y = base + row;
      if constexpr (ROWS && MODE == kXeItem) {
        pf[k] = y < yhi ? Y4[rows[y] * V4 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        pf[k] = y < yhi ? Y4[y * V4 + c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto store_tile = [&](float* dst) {
#pragma unroll
    for (int k = 0; k < NPF; ++k) {
      const int f = threadIdx.x + k * kXeThreads;
      const int row = f / V4;
      const int c4 = f - row * V4;
      float2* p = reinterpret_cast<float2*>(dst + row * LDR + 4 * c4);
      p[0] = make_float2(pf[k].x, pf[k].y);
      p[1] = make_float2(pf[k].z, pf[k].w);
    }
  };
  auto stage_meta = [&](int64_t base, int buf) {
    if constexpr (MODE == kXeItem) {
      if (threadIdx.x < TI) {
        const int64_t q = base + threadIdx.x;
        s_lse[buf][threadIdx.x] = q < yhi ? lse[q] : 0.f;
        s_tgt[buf][threadIdx.x] = q < yhi ? target[q] : (int64_t)-1;
      }
    }
  };

  const int64_t ntile = (yhi - ylo + TI - 1) / TI;
  load_tile(ylo);
  store_tile(tile[0]);
  stage_meta(ylo, 0);
  __syncthreads();
  int cur = 0;
  for (int64_t t = 0; t < ntile; ++t) {
    const int64_t base = ylo + t * TI;
    const bool more = t + 1 < ntile;
    if (more) load_tile(base + TI);            // global loads in flight under the MFMAs
#pragma unroll 1
    for (int sub = 0; sub < NT; ++sub) {
      floatx16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const float* arow = tile[cur] + (32 * sub + j) * LDR + 2 * h;
#pragma unroll
      for (int s2 = 0; s2 < D / 4; ++s2) {
        const float2 a = *reinterpret_cast<const float2*>(arow + 4 * s2);
        acc = mfma_32x32x2(a.x, ub[2 * s2], acc);
        acc = mfma_32x32x2(a.y, ub[2 * s2 + 1], acc);
      }
      const int64_t sb = base + 32 * sub;
      if constexpr (MODE == kXeFwd) {
        float best = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t item = sb + (r & 3) + 8 * (r >> 2) + 4 * h;
          acc[r] = item < yhi ? acc[r] : -INFINITY;
          tl = item == tq ? acc[r] : tl;
          best = fmaxf(best, acc[r]);
        }
        const float mn = fmaxf(m, best);
        const float mref = mn == -INFINITY ? 0.f : mn;   // no valid item yet: keep sum 0
        float add = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) add += __expf(acc[r] - mref);
        s = s * __expf(m - mref) + add;
        m = mn;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
          const int64_t y = sb + row;
          float l = lq;
          int64_t tg = tq, item = y;
          if constexpr (MODE == kXeItem) {
            l = s_lse[cur][32 * sub + row];
            tg = s_tgt[cur][32 * sub + row];
            item = x;
          }
          const float p = __expf(acc[r] - l) - (item == tg ? 1.f : 0.f);
          acc[r] = (xv && y < yhi) ? p * scale : 0.f;
        }
        // out[fixed x][c] += sum over the sub-tile's swept rows of w[y][x] * Y[y][c]
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float* brow =
              tile[cur] + (32 * sub + (r & 3) + 8 * (r >> 2) + 4 * h) * LDR + j;
#pragma unroll
          for (int cb = 0; cb < NCB; ++cb)
            oacc[cb] = mfma_32x32x2(acc[r], brow[32 * cb], oacc[cb]);
        }
      }
    }
    if (more) {
      store_tile(tile[cur ^ 1]);
      stage_meta(base + TI, cur ^ 1);
    }
    __syncthreads();
    cur ^= 1;
  }

  if constexpr (MODE == kXeFwd) {
    // merge the two item halves of each query: half 0's sum first
    const float om = __shfl(m, j + 32, 64);
    const float os = __shfl(s, j + 32, 64);
    const float ot = __shfl(tl, j + 32, 64);
    if (h == 0 && xv) {
      const float mn = fmaxf(m, om);
      const float mref = mn == -INFINITY ? 0.f : mn;
      const int64_t o = (int64_t)blockIdx.y * B + x;
      pm[o] = mn;
      ps[o] = s * __expf(m - mref) + os * __expf(om - mref);
      pt[o] = fmaxf(tl, ot);
    }
  } else {
    // oacc[cb][r]: fixed row (r&3) + 8*(r>>2) + 4h of the wave, column 32*cb + j
    float* dst = out + (MODE == kXeQuery ? (int64_t)blockIdx.y * B * D : (int64_t)0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t xr = xb + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (xr < NX) {
        const bool live = !ROWS || MODE == kXeItem || xr < nx;    // a dead query's row: zeros
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          dst[xr * D + 32 * cb + j] = live ? oacc[cb][r] : 0.f;
      }
    }
  }
}

// Fold the item splits' partials per query, ascending split order.
__global__ __launch_bounds__(256) void xent_finish_kernel(
    int64_t B, int S, const float* __restrict__ pm, const float* __restrict__ ps,
    const float* __restrict__ pt, float* __restrict__ lse, float* __restrict__ loss_rows,
    const int32_t* __restrict__ n_dev) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= B) return;
  if (n_dev && q >= (int64_t)n_dev[0]) {      // K17: a query past the count has no partials
    lse[q] = 0.f;
    loss_rows[q] = 0.f;
    return;
  }
  float m = -INFINITY, s = 0.f, tl = -INFINITY;
  for (int k = 0; k < S; ++k) {
    const int64_t o = (int64_t)k * B + q;
    const float om = pm[o];
    const float mn = fmaxf(m, om);
    const float mref = mn == -INFINITY ? 0.f : mn;
    s = s * __expf(m - mref) + ps[o] * __expf(om - mref);
    m = mn;
    tl = fmaxf(tl, pt[o]);
  }
  const float l = m + logf(s);
  lse[q] = l;
  loss_rows[q] = l - tl;
}

// out[e] = sum over the splits of part[k][e], ascending k (n4 float4 elements per split).
__global__ __launch_bounds__(256) void xent_sum_kernel(int64_t n4, int S,
                                                       const float4* __restrict__ part,
                                                       float4* __restrict__ out, int d4,
                                                       const int32_t* __restrict__ n_dev) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n4) return;
  if (n_dev && e / d4 >= (int64_t)n_dev[0]) {   // K17: the row of a query past the count
    out[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  float4 a = part[e];
  for (int k = 1; k < S; ++k) {
    const float4 b = part[(int64_t)k * n4 + e];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
  }
  out[e] = a;
}

// The item split actually used: `splits` <= 0 = auto, a pure function of (B, I) —
// about two workgroups per CU, at least eight 64-item tiles per split, at most 128 —
// otherwise the request, clamped so that a span is a whole number of tiles and at
// least one. *span gets the items per split.
static int xe_resolve(int64_t B, int64_t I, int32_t splits, int64_t* span) {
  const int64_t tiles = (I + kXeTile - 1) / kXeTile;
  int64_t n = splits;
  if (n <= 0) {
    const int64_t nqb = (B + 127) / 128;
    n = (512 + nqb - 1) / nqb;
    n = n < (tiles + 7) / 8 ? n : (tiles + 7) / 8;
    n = n < 128 ? n : 128;
  }
  n = n < 65535 ? n : 65535;
  n = n < tiles ? n : tiles;
  n = n > 1 ? n : 1;
  const int64_t st = (tiles + n - 1) / n;
  *span = st * kXeTile;
  return (int)((tiles + st - 1) / st);
}

}  // namespace mirec

using namespace mirec;

extern "C" int32_t mirec_full_ce_splits(int64_t B, int64_t I, int32_t d, int32_t splits) {
  (void)d;
  if (B <= 0 || I <= 0) return 1;
  int64_t span;
  return xe_resolve(B, I, splits, &span);
}

extern "C" size_t mirec_full_ce_workspace_size(int64_t B, int64_t I, int32_t d,
                                               int32_t splits) {
  if (B <= 0 || I <= 0 || d <= 0) return 256;
  int64_t span;
  const size_t S = (size_t)xe_resolve(B, I, splits, &span);
  const size_t fwd = 3 * S * (size_t)B * sizeof(float);
  const size_t bwd = S > 1 ? S * (size_t)B * (size_t)d * sizeof(float) : 0;
  return (fwd > bwd ? fwd : bwd) + 256;
}

#define MIREC_XE_LAUNCH(DD, MODE, grd, ...)                                               \
  if (rows)                                                                               \
    hipLaunchKernelGGL((xent_kernel<DD, MODE, true>), grd, dim3(kXeThreads), 0, st,       \
                       __VA_ARGS__, rows, n_dev);                                         \
  else                                                                                    \
    hipLaunchKernelGGL((xent_kernel<DD, MODE, false>), grd, dim3(kXeThreads), 0, st,      \
                       __VA_ARGS__, (const int64_t*)nullptr, (const int32_t*)nullptr)
#define MIREC_XE_SWITCH(what, MODE, grd, ...)                                             \
  switch (d) {                                                                            \
    case 32: MIREC_XE_LAUNCH(32, MODE, grd, __VA_ARGS__); break;                          \
    case 64: MIREC_XE_LAUNCH(64, MODE, grd, __VA_ARGS__); break;                          \
    case 128: MIREC_XE_LAUNCH(128, MODE, grd, __VA_ARGS__); break;                        \
    case 256: MIREC_XE_LAUNCH(256, MODE, grd, __VA_ARGS__); break;                        \
    default:                                                                              \
      set_error("%s: hidden size %d not in {32,64,128,256}", what, d);                    \
      return -1;                                                                          \
  }

// S: the query matrix; B queries — its rows 0 .. B-1 (rows null), or its rows rows[r] of
// which only the first min(B, *n_dev) exist (K17).
static int xe_fwd(const float* S, int64_t B, const int64_t* rows, const int32_t* n_dev,
                  const float* E, int64_t I, int32_t d, const int64_t* target, int32_t splits,
                  float* lse, float* loss_rows, void* workspace, void* stream,
                  const char* what) {
  if (B == 0) return 0;
  if (!S || !E || !target || !lse || !loss_rows || !workspace || B < 0 || I <= 0) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  int64_t span;
  const int ns = xe_resolve(B, I, splits, &span);
  float* pm = (float*)workspace;
  float* ps = pm + (size_t)ns * B;
  float* pt = ps + (size_t)ns * B;
  const dim3 grd((unsigned)((B + 127) / 128), (unsigned)ns);
  hipStream_t st = (hipStream_t)stream;
  MIREC_XE_SWITCH(what, kXeFwd, grd, S, B, E, I, target, (const float*)nullptr,
                  (const float*)nullptr, B, span, (float*)nullptr, pm, ps, pt)
  hipLaunchKernelGGL(xent_finish_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, B,
                     ns, pm, ps, pt, lse, loss_rows, rows ? n_dev : (const int32_t*)nullptr);
  return launch_status(what);
}

static int xe_bwd(const float* S, int64_t B, const int64_t* rows, const int32_t* n_dev,
                  const float* E, int64_t I, int32_t d, const int64_t* target, const float* lse,
                  const float* g_dev, int32_t splits, float* gS, float* dE, void* workspace,
                  void* stream, const char* what) {
  if (B == 0) return 0;
  if (!S || !E || !target || !lse || !g_dev || !gS || !dE || !workspace || B < 0 || I <= 0) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  int64_t span;
  const int ns = xe_resolve(B, I, splits, &span);
  float* part = ns > 1 ? (float*)workspace : gS;
  const dim3 gq((unsigned)((B + 127) / 128), (unsigned)ns);
  const dim3 gi((unsigned)((I + 127) / 128));
  const int64_t qspan = (B + kXeTile - 1) / kXeTile * kXeTile;
  hipStream_t st = (hipStream_t)stream;
  MIREC_XE_SWITCH(what, kXeQuery, gq, S, B, E, I, target, lse, g_dev, B, span, part,
                  (float*)nullptr, (float*)nullptr, (float*)nullptr)
  if (ns > 1) {
    const int64_t n4 = B * d / 4;
    hipLaunchKernelGGL(xent_sum_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, n4,
                       ns, (const float4*)part, (float4*)gS, d / 4,
                       rows ? n_dev : (const int32_t*)nullptr);
  }
  MIREC_XE_SWITCH(what, kXeItem, gi, E, I, S, B, target, lse, g_dev, B, qspan, dE,
                  (float*)nullptr, (float*)nullptr, (float*)nullptr)
  return launch_status(what);
}

extern "C" int mirec_full_ce_fwd_f32(const float* S, int64_t B, const float* E, int64_t I,
                                     int32_t d, const int64_t* target, int32_t splits,
                                     float* lse, float* loss_rows, void* workspace,
                                     void* stream) {
  return xe_fwd(S, B, nullptr, nullptr, E, I, d, target, splits, lse, loss_rows, workspace,
                stream, "mirec_full_ce_fwd_f32");
}

extern "C" int mirec_full_ce_bwd_f32(const float* S, int64_t B, const float* E, int64_t I,
                                     int32_t d, const int64_t* target, const float* lse,
                                     const float* g_dev, int32_t splits, float* gS, float* dE,
                                     void* workspace, void* stream) {
  return xe_bwd(S, B, nullptr, nullptr, E, I, d, target, lse, g_dev, splits, gS, dE, workspace,
                stream, "mirec_full_ce_bwd_f32");
}

extern "C" int mirec_rows_ce_fwd_f32(const float* X, int64_t n_x, const int64_t* row,
                                          int64_t R, const int32_t* n_rows_dev, const float* E,
                                          int64_t I, int32_t d, const int64_t* target,
                                          int32_t splits, float* lse, float* loss_rows,
                                          void* workspace, void* stream) {
  if (R > 0 && (!row || n_x <= 0)) {
    set_error("mirec_rows_ce_fwd_f32: bad arguments");
    return -1;
  }
  return xe_fwd(X, R, row, n_rows_dev, E, I, d, target, splits, lse, loss_rows, workspace,
                stream, "mirec_rows_ce_fwd_f32");
}

extern "C" int mirec_rows_ce_bwd_f32(const float* X, int64_t n_x, const int64_t* row,
                                          int64_t R, const int32_t* n_rows_dev, const float* E,
                                          int64_t I, int32_t d, const int64_t* target,
                                          const float* lse, const float* g_dev, int32_t splits,
                                          float* gS, float* dE, void* workspace, void* stream) {
  if (R > 0 && (!row || n_x <= 0)) {
    set_error("mirec_rows_ce_bwd_f32: bad arguments");
    return -1;
  }
  return xe_bwd(X, R, row, n_rows_dev, E, I, d, target, lse, g_dev, splits, gS, dE, workspace,
                stream, "mirec_rows_ce_bwd_f32");
}
