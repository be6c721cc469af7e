// K18 — xDeepFM's Compressed Interaction Network (reference xdeepfm.py:116-169) on fp32 MFMA.
// One layer, with X0 [B, m, D], Xk [B, H, D] (X_0 = X0), W [N, H m] (the Conv1d weight
// without its trailing 1) and b [N]:
//   out[b, n, d] = b[n] + sum_{h < H} sum_{j < m} W[n, h m + j] Xk[b, h, d] X0[b, j, d]
// The reference forms z = einsum('bmd,bhd->bhmd') of shape [B, H m, D] (199 - 256 MB a layer
// at B = 2048, m = 39, D = 16) and autograd keeps it. Seen over the R = B D (sample,
// dimension) rows r = b D + d, a layer is the GEMM [R, H m] x [H m, N] whose A operand
// Xk[r, h] X0[r, j] is a product of two short rows: it is formed in registers, z never
// exists.
//
// The channels of out split by two numbers (n_hid, dir0): channels [0, n_hid) go on as
// X_{k+1} [B, n_hid, D]; channels [dir0, N) are pooled, pooled[b, pool_off + n - dir0] =
// sum_d out[b, n, d] (a column block of the [B, final_len] result). direct: True has
// (N, 0) and (0, 0) for the last layer, direct: False (N/2, N/2) and (0, 0).
//
// The K space is walked one h at a time, j padded to 16 NU = the 16-wide tiles of m: per h
// the weight slab W[:, h m .. h m + m) is staged zero-padded into LDS (double-buffered, one
// barrier per h) and the workgroup's four waves, one 16-row slab each, run the shared slab
// product (mfma.h) against it.
//
//   K18a cin_fwd_kernel    workgroup = floor(64 / D) whole samples (<= 64 rows). Lane
//                          (li, lk) keeps X0[r, 16u + 4lk ..+3] for its row in registers
//                          and reads Xk[r, h] one h ahead; A = X0 regs * Xk[r, h] (one
//                          v_mul per float of the A operand, reused over the N / 16 column
//                          tiles). Epilogue: out + bias goes through LDS (the staging
//                          buffers, free by then); X_{k+1} is written coalesced and each
//                          pooled value is summed over d = 0 .. D-1 in that order by one
//                          lane — whole samples per workgroup, so no sum crosses workgroups.
//   K18b cin_bwd_kernel    G[r, n] = dX_{k+1}[b, n, d] (n < n_hid) + g_pooled[b, ..] (n >=
//                          dir0) as the A rows; per h the slab W[:, h m ..]^T is staged and
//                          T[r, (h, j)] = sum_n G[r, n] W[n, h m + j] lands in NU
//                          accumulators, which are consumed at once: dXk[r, h] = sum_j T
//                          X0[r, j] (the tiles in order, then an xor butterfly over the 16
//                          lanes) and dX0[r, j] += T Xk[r, h] in registers over h ascending.
//                          Layer 0 (Xk = X0) adds dXk into the same registers. dX0 is
//                          written or added to (the layers are launched last to first).
//   K18c cin_wgrad_kernel  dW[n, h m + j] = sum_r G[r, n] Xk[r, h] X0[r, j]: a wave owns a
//                          unit (h, 16 columns j) and every n tile; the workgroup's four
//                          units share the G and X0 rows, staged through LDS 32 rows at a
//                          time. One more wave sums db[n] = sum_r G from the staged rows
//                          (float64 running sums, rows in order).
//                          blockIdx.y splits the rows; split s stores its partial
//                          [dW | db] and mirec_linear_grad_finish_f32 adds them in split
//                          order. The number of splits is capped, so the scratch does not
//                          grow with B.
//
// Every sum has an order fixed by the shapes: the MFMA k order (h ascending, then the slab
// product's order; K18a adds every 16 slabs' accumulators into a second set), the pooled sum over d ascending, dX0 over h ascending and the layers in
// launch order, the weight gradient over the rows in order and the splits in order. No
// float atomics.
//
// Resources: dynamic LDS, K18a 2 x 16 NC x 68 floats (NC = column tiles of N, <= 139264 B),
// K18b 2 x 16 NU x (16 NK + 4) floats (<= 133120 B), K18c 2 x (16 NC + 64) x 36 floats
// (<= 92160 B). Registers (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; VGPR +
// AGPR) at N = 100, m = 39 (NC = 8, NU = 3): K18a 256 + 47, K18b 256 + 120, K18c 171 + 48, no
// scratch. The widest forms spill to scratch: K18a at NC = 16, NU = 4 (296 B per lane), K18b at
// NK = 16 with NU >= 2 and NK = 12 with NU = 4 (124 - 788 B); no other form does.
#include "common.h"
#include "mfma.h"
#include "rowsplit.h"

#include <algorithm>

namespace mirec {

constexpr int kCinThreads = 256;          // four waves, one 16-row slab each
constexpr int kCinWaves = kCinThreads / 64;
constexpr int kCinRows = 16 * kCinWaves;  // rows of a workgroup's pass
constexpr int kCinKP = 68;                // K18a's LDS row stride: 16 x 4 columns j + 4
constexpr int kCinFlush = 16;             // K18a: slabs (h) per first-level accumulator

// the upstream gradient of a layer's output, never stored: see the header
struct CinGrad {
  const float* dXn;   // [B, n_hid, D] or NULL
  const float* gp;    // g_pooled [B, pool_ld]
  int n_hid, dir0, N, pool_off, pool_ld;
  __device__ __forceinline__ float at(int64_t b, int d, int D, int n) const {
    float g = 0.f;
    if (dXn && n < n_hid) g = dXn[(b * n_hid + n) * D + d];
    if (n >= dir0 && n < N) g += gp[b * pool_ld + pool_off + (n - dir0)];
    return g;
  }
};

// ---------------------------------------------------------------- K18a
template <int NC, int NU>
__global__ __launch_bounds__(kCinThreads) void cin_fwd_kernel(
    const float* __restrict__ X0, const float* __restrict__ Xk, int64_t B, int m, int H, int D,
    const float* __restrict__ W, const float* __restrict__ bias, int N, int n_hid, int dir0,
    float* __restrict__ Xn, float* __restrict__ pooled, int pool_off, int pool_ld,
    int64_t chunks) {
  constexpr int BUF = 16 * NC * kCinKP, RS = 16 * NC + 1, NST = NC * NU;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 x [16 NC][kCinKP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int S = kCinRows / D, rows_c = S * D, K = H * m;
  // element tid + 256 q of the [16 NC][16 NU] slab: row n, column j
  auto load_stage = [&](float (&st)[NST], int h) {
#pragma unroll
    for (int q = 0; q < NST; ++q) {
      const int e = tid + kCinThreads * q, n = e / (16 * NU), j = e % (16 * NU);
      st[q] = (n < N && j < m) ? W[(int64_t)n * K + h * m + j] : 0.f;
    }
  };
  auto store_stage = [&](const float (&st)[NST], float* buf) {
#pragma unroll
    for (int q = 0; q < NST; ++q) {
      const int e = tid + kCinThreads * q, n = e / (16 * NU), j = e % (16 * NU);
      buf[n * kCinKP + j] = st[q];
    }
  };
  for (int64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    const int64_t b0 = ch * S;
    const int rr = 16 * w + li, sb = rr / D, d = rr - sb * D;
    const int64_t b = b0 + sb;
    const bool ok = rr < rows_c && b < B;
    float4 x0r[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 16 * u + 4 * lk + e;
        v[e] = (ok && j < m) ? X0[(b * m + j) * D + d] : 0.f;
      }
      x0r[u] = make_float4(v[0], v[1], v[2], v[3]);
    }
    const float* xkp = Xk + (ok ? b * H * D + d : 0);
    float xk = ok ? xkp[0] : 0.f;
    // two levels: acc takes kCinFlush slabs (h), then goes into tot — an fp32 running sum
    // over all H m <= 16,384 products would carry sqrt(K) times one rounding
    floatx4 acc[NC], tot[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = tot[c] = floatx4{0.f, 0.f, 0.f, 0.f};
    float st[NST];
    load_stage(st, 0);
    store_stage(st, smem);
    __syncthreads();
    for (int h = 0; h < H; ++h) {
      const bool more = h + 1 < H;
      float xkn = 0.f;
      if (more) {
        load_stage(st, h + 1);
        xkn = ok ? xkp[(int64_t)(h + 1) * D] : 0.f;
      }
      float4 a[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u)
        a[u] = make_float4(x0r[u].x * xk, x0r[u].y * xk, x0r[u].z * xk, x0r[u].w * xk);
      mfma_slab_acc<NU, NC, kCinKP>(a, lds_ptr(smem + (h & 1) * BUF), li, lk, acc);
      if (more) store_stage(st, smem + ((h + 1) & 1) * BUF);
      xk = xkn;
      if ((h + 1) % kCinFlush == 0 || !more) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          tot[c] += acc[c];
          acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
      }
      __syncthreads();
    }
    // C layout: tot[c][i] = out[row 16 w + 4lk + i][16c + li] before the bias
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int n = 16 * c + li;
      const float bv = n < N ? bias[n] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) smem[(16 * w + 4 * lk + i) * RS + n] = tot[c][i] + bv;
    }
    __syncthreads();
    const int nsv = (int)std::min<int64_t>(S, B - b0);
    if (n_hid > 0) {
      const int per = n_hid * D;
      for (int idx = tid; idx < nsv * per; idx += kCinThreads) {
        const int s = idx / per, rem = idx - s * per, n = rem / D, dd = rem - n * D;
        Xn[(b0 + s) * per + rem] = smem[(s * D + dd) * RS + n];
      }
    }
    const int nd = N - dir0;
    for (int idx = tid; idx < nsv * nd; idx += kCinThreads) {
      const int s = idx / nd, q = idx - s * nd;
      const float* col = smem + (s * D) * RS + dir0 + q;
      float sum = col[0];
      for (int dd = 1; dd < D; ++dd) sum += col[dd * RS];
      pooled[(b0 + s) * pool_ld + pool_off + q] = sum;
    }
    __syncthreads();                      // the next chunk stages into the same floats
  }
}

// ---------------------------------------------------------------- K18b
template <int NK, int NU>
__global__ __launch_bounds__(kCinThreads) void cin_bwd_kernel(
    const float* __restrict__ X0, const float* __restrict__ Xk, int64_t R, int m, int H, int D,
    const float* __restrict__ W, const CinGrad g, float* __restrict__ dXk,
    float* __restrict__ dX0, int accumulate, int64_t groups) {
  constexpr int KP = 16 * NK + 4, BUF = 16 * NU * KP, NST = NK * NU;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 x [16 NU][KP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int K = H * m, N = g.N;
  // element tid + 256 q of the transposed slab: row j (fastest over the lanes), column n
  auto load_stage = [&](float (&st)[NST], int h) {
#pragma unroll
    for (int q = 0; q < NST; ++q) {
      const int e = tid + kCinThreads * q, n = e / (16 * NU), j = e % (16 * NU);
      st[q] = (n < N && j < m) ? W[(int64_t)n * K + h * m + j] : 0.f;
    }
  };
  auto store_stage = [&](const float (&st)[NST], float* buf) {
#pragma unroll
    for (int q = 0; q < NST; ++q) {
      const int e = tid + kCinThreads * q, n = e / (16 * NU), j = e % (16 * NU);
      buf[j * KP + n] = st[q];
    }
  };
  for (int64_t sg = blockIdx.x; sg < groups; sg += gridDim.x) {
    const int64_t base = kCinRows * sg + 16 * w;
    // A rows: lane (li, lk) holds G[base + li][16u + 4lk .. +3]
    float4 a[NK];
    {
      const int64_t r = base + li;
      const bool ok = r < R;
      const int64_t b = ok ? r / D : 0;
      const int d = ok ? (int)(r - b * D) : 0;
#pragma unroll
      for (int u = 0; u < NK; ++u) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = ok ? g.at(b, d, D, 16 * u + 4 * lk + e) : 0.f;
        a[u] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
    // C layout rows base + 4lk + i, columns j = 16c + li
    bool okc[4];
    int64_t bc[4];
    int dc[4];
    float x0c[NU][4], dx0[NU][4], xk[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = base + 4 * lk + i;
      okc[i] = r < R;
      bc[i] = okc[i] ? r / D : 0;
      dc[i] = okc[i] ? (int)(r - bc[i] * D) : 0;
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        const int j = 16 * c + li;
        x0c[c][i] = (okc[i] && j < m) ? X0[(bc[i] * m + j) * D + dc[i]] : 0.f;
        dx0[c][i] = 0.f;
      }
      xk[i] = okc[i] ? Xk[bc[i] * H * D + dc[i]] : 0.f;
    }
    float st[NST];
    load_stage(st, 0);
    store_stage(st, smem);
    __syncthreads();
    for (int h = 0; h < H; ++h) {
      const bool more = h + 1 < H;
      float xkn[4] = {0.f, 0.f, 0.f, 0.f};
      if (more) {
        load_stage(st, h + 1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
          xkn[i] = okc[i] ? Xk[(bc[i] * H + h + 1) * D + dc[i]] : 0.f;
      }
      floatx4 acc[NU];
      mfma_slab<NK, NU, KP>(a, lds_ptr(smem + (h & 1) * BUF), li, lk, acc);
      // acc[c][i] = T[base + 4lk + i][(h, 16c + li)]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NU; ++c) {
          s = fmaf(acc[c][i], x0c[c][i], s);
          dx0[c][i] = fmaf(acc[c][i], xk[i], dx0[c][i]);
        }
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) s += __shfl_xor(s, off, 64);
        if (dXk) {
          if (li == i && okc[i]) dXk[(bc[i] * H + h) * D + dc[i]] = s;
        } else {                          // layer 0: Xk = X0, column j = h takes this term too
#pragma unroll
          for (int c = 0; c < NU; ++c)
            if (c == (h >> 4) && li == (h & 15)) dx0[c][i] += s;
        }
      }
      if (more) store_stage(st, smem + ((h + 1) & 1) * BUF);
#pragma unroll
      for (int i = 0; i < 4; ++i) xk[i] = xkn[i];
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        const int j = 16 * c + li;
        if (okc[i] && j < m) {
          float* o = dX0 + (bc[i] * m + j) * D + dc[i];
          *o = accumulate ? *o + dx0[c][i] : dx0[c][i];
        }
      }
  }
}

// ---------------------------------------------------------------- K18c
constexpr int kCinWgRows = 32;            // rows staged at a time
constexpr int kCinWgLS = 36;              // their LDS stride: 16 lanes x 36 floats hit 16 banks apart

template <int NC>
__global__ __launch_bounds__(kCinThreads) void cin_wgrad_kernel(
    const float* __restrict__ X0, const float* __restrict__ Xk, int64_t R, int m, int H, int D,
    const CinGrad g, int64_t rows_per_split, float* __restrict__ partials, int64_t stride,
    int64_t db_off) {
  constexpr int GB = 16 * NC * kCinWgLS, XB = 64 * kCinWgLS, BUF = GB + XB;
  constexpr int NG = 16 * NC * kCinWgRows / kCinThreads, NX = 64 * kCinWgRows / kCinThreads;
  extern __shared__ __attribute__((aligned(16))) float smem[];   // 2 x (Gs[16 NC][36] | X0s[64][36])
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int N = g.N, K = H * m, NU = (m + 15) / 16, units = H * NU;
  const int unit = kCinWaves * blockIdx.x + w;
  const bool is_db = unit == units, active = unit < units;
  const int h = active ? unit / NU : 0, jt = active ? unit % NU : 0;
  const int64_t r_beg = (int64_t)blockIdx.y * rows_per_split;
  const int64_t r_end = std::min<int64_t>(R, r_beg + rows_per_split);
  // staging: thread (row tid % 32, columns tid / 32 + 8 q) of the chunk
  const int srow = tid % kCinWgRows, scol = tid / kCinWgRows;
  auto load_stage = [&](float (&sg)[NG], float (&sx)[NX], int64_t r0) {
    const int64_t r = r0 + srow;
    const bool ok = r < r_end;
    const int64_t b = ok ? r / D : 0;
    const int d = ok ? (int)(r - b * D) : 0;
#pragma unroll
    for (int q = 0; q < NG; ++q) sg[q] = ok ? g.at(b, d, D, scol + 8 * q) : 0.f;
#pragma unroll
    for (int q = 0; q < NX; ++q) {
      const int j = scol + 8 * q;
      sx[q] = (ok && j < m) ? X0[(b * m + j) * D + d] : 0.f;
    }
  };
  auto store_stage = [&](const float (&sg)[NG], const float (&sx)[NX], float* buf) {
#pragma unroll
    for (int q = 0; q < NG; ++q) buf[(scol + 8 * q) * kCinWgLS + srow] = sg[q];
#pragma unroll
    for (int q = 0; q < NX; ++q) buf[GB + (scol + 8 * q) * kCinWgLS + srow] = sx[q];
  };
  // the wave's Xk[r, h] for rows r0 + 4q + lk
  auto load_xk = [&](float (&xv)[8], int64_t r0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int64_t r = r0 + 4 * q + lk;
      float v = 0.f;
      if (active && r < r_end) {
        const int64_t b = r / D;
        v = Xk[(b * H + h) * D + (r - b * D)];
      }
      xv[q] = v;
    }
  };
  // the bias unit: lane l sums the columns n = l + 64 t of G over the rows in order, in
  // float64 (a column of same-signed terms would lose bits in an fp32 running sum)
  constexpr int NT = (16 * NC + 63) / 64;
  double dsum[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) dsum[t] = 0.0;
  floatx4 acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
  float sg[NG], sx[NX], xv[8];
  load_stage(sg, sx, r_beg);
  load_xk(xv, r_beg);
  store_stage(sg, sx, smem);
  __syncthreads();
  int it = 0;
  for (int64_t r0 = r_beg; r0 < r_end; r0 += kCinWgRows, ++it) {
    const bool more = r0 + kCinWgRows < r_end;
    float xn[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (more) {
      load_stage(sg, sx, r0 + kCinWgRows);
      load_xk(xn, r0 + kCinWgRows);
    }
    if (active) {
      const float* Gs = smem + (it & 1) * BUF;
      const float* Xs = Gs + GB;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        // A[li = n][lk = row] = G[r0 + 4q + lk][16c + li]; B[lk][li] = Xk[row, h] X0[row, 16 jt + li]
        const float bv = xv[q] * Xs[(16 * jt + li) * kCinWgLS + 4 * q + lk];
        float av[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) av[c] = Gs[(16 * c + li) * kCinWgLS + 4 * q + lk];
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = mfma_16x16x4(av[c], bv, acc[c]);
      }
    }
    if (is_db) {
      const float* Gs = smem + (it & 1) * BUF;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int n = lane + 64 * t;
        if (n < 16 * NC) {
#pragma unroll
          for (int q = 0; q < kCinWgRows / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(&Gs[n * kCinWgLS + 4 * q]);
            dsum[t] += (double)v.x;
            dsum[t] += (double)v.y;
            dsum[t] += (double)v.z;
            dsum[t] += (double)v.w;
          }
        }
      }
    }
    if (more) store_stage(sg, sx, smem + ((it + 1) & 1) * BUF);
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = xn[q];
    __syncthreads();
  }
  float* P = partials + (int64_t)blockIdx.y * stride;
  if (is_db) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (lane + 64 * t < N) P[db_off + lane + 64 * t] = (float)dsum[t];
  }
  if (!active) return;
  // C layout: acc[c][i] = P[n = 16c + 4lk + i][column 16 jt + li]
  const int j = 16 * jt + li;
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = 16 * c + 4 * lk + i;
      if (n < N && j < m) P[(int64_t)n * K + h * m + j] = acc[c][i];
    }
}

// ---------------------------------------------------------------- host side
// mirec_cin_grid_cap: most workgroups K18a / K18b launch (0: the CUs decide)
static GridCap g_cin_cap;

// the built tile counts of N: 16 NC >= N
static int cin_nc(int N) {
  const int t = (N + 15) / 16;
  return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : t <= 12 ? 12 : 16;
}

template <int NC, int NU>
static int launch_cin_fwd(const float* X0, const float* Xk, int64_t B, int m, int H, int D,
                          const float* W, const float* b, int N, int n_hid, int dir0, float* Xn,
                          float* pooled, int pool_off, int pool_ld, hipStream_t st,
                          const char* what) {
  constexpr size_t lds = (size_t)2 * 16 * NC * kCinKP * sizeof(float);
  static_assert(2 * 16 * NC * kCinKP >= kCinRows * (16 * NC + 1), "the epilogue tile fits");
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(cin_fwd_kernel<NC, NU>, kCinThreads, lds, cache, &per_cu, what)) return -1;
  const int S = kCinRows / D;
  const int64_t chunks = (B + S - 1) / S;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((cin_fwd_kernel<NC, NU>), dim3(g_cin_cap.grid(chunks, most)),
                     dim3(kCinThreads), lds, st, X0, Xk, B, m, H, D, W, b, N, n_hid, dir0, Xn,
                     pooled, pool_off, pool_ld, chunks);
  return launch_status(what);
}

template <int NK, int NU>
static int launch_cin_bwd(const float* X0, const float* Xk, int64_t R, int m, int H, int D,
                          const float* W, const CinGrad& g, float* dXk, float* dX0,
                          int accumulate, hipStream_t st, const char* what) {
  constexpr size_t lds = (size_t)2 * 16 * NU * (16 * NK + 4) * sizeof(float);
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(cin_bwd_kernel<NK, NU>, kCinThreads, lds, cache, &per_cu, what)) return -1;
  const int64_t groups = (R + kCinRows - 1) / kCinRows;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((cin_bwd_kernel<NK, NU>), dim3(g_cin_cap.grid(groups, most)),
                     dim3(kCinThreads), lds, st, X0, Xk, R, m, H, D, W, g, dXk, dX0, accumulate,
                     groups);
  return launch_status(what);
}

template <int NC>
static int launch_cin_wgrad(const float* X0, const float* Xk, int64_t R, int m, int H, int D,
                            const CinGrad& g, int64_t rows, int splits, float* partials,
                            int64_t stride, int64_t db_off, hipStream_t st, const char* what) {
  constexpr size_t lds = (size_t)2 * (16 * NC + 64) * kCinWgLS * sizeof(float);
  static int cache[kMaxDev] = {};
  if (prepare_launch(cin_wgrad_kernel<NC>, kCinThreads, lds, cache, nullptr, what)) return -1;
  const int units = H * ((m + 15) / 16) + 1;
  hipLaunchKernelGGL((cin_wgrad_kernel<NC>),
                     dim3((unsigned)((units + kCinWaves - 1) / kCinWaves), (unsigned)splits),
                     dim3(kCinThreads), lds, st, X0, Xk, R, m, H, D, g, rows, partials, stride,
                     db_off);
  return launch_status(what);
}

// K18c's row split: enough workgroups to fill the chip, at most kCinWgMaxSplits partials, each
// over a multiple of 32 rows and at least kCinWgMinRows of them
constexpr int kCinWgMaxSplits = 32;
constexpr int64_t kCinWgMinRows = 256;
constexpr int kCinWgTarget = 512;         // workgroups wanted

static RowSplit cin_wgrad_split(int64_t R, int m, int H) {
  const int units = H * ((m + 15) / 16) + 1;
  const int groups = (units + kCinWaves - 1) / kCinWaves;
  const int want = std::min(kCinWgMaxSplits, std::max(1, kCinWgTarget / groups));
  return row_split(R, want, kCinWgRows, kCinWgMinRows);
}

static int cin_shape_error(const char* what, int32_t m, int32_t H, int32_t D, int32_t N) {
  set_error("%s: shape m %d, H %d, D %d, N %d is not built (m 2..64, H 1..256, D 1..64, "
            "N 2..256)", what, m, H, D, N);
  return -1;
}

static bool cin_channels_ok(int N, int n_hid, int dir0) {
  return n_hid >= 0 && n_hid <= N && dir0 >= 0 && dir0 <= N;
}

}  // namespace mirec

using namespace mirec;

#define MIREC_CIN_TILES(F, U) F(1, U) F(2, U) F(4, U) F(8, U) F(12, U) F(16, U)
#define MIREC_CIN_FORMS(F) MIREC_CIN_TILES(F, 1) MIREC_CIN_TILES(F, 2) MIREC_CIN_TILES(F, 3) \
  MIREC_CIN_TILES(F, 4)

extern "C" int32_t mirec_cin_grid_cap(int32_t workgroups) {
  return g_cin_cap.exchange(workgroups);
}

extern "C" int mirec_cin_shape_ok(int32_t m, int32_t H, int32_t D, int32_t N) {
  return m >= 2 && m <= 64 && H >= 1 && H <= 256 && D >= 1 && D <= 64 && N >= 2 && N <= 256;
}

extern "C" int mirec_cin_layer_fwd_f32(const float* X0, const float* Xk, int64_t B, int32_t m,
                                       int32_t H, int32_t D, const float* W, const float* b,
                                       int32_t N, int32_t n_hid, int32_t dir0, float* Xn,
                                       float* pooled, int32_t pool_off, int32_t pool_ld,
                                       void* stream) {
  const char* what = "mirec_cin_layer_fwd_f32";
  if (!mirec_cin_shape_ok(m, H, D, N)) return cin_shape_error(what, m, H, D, N);
  if (B < 0 || !X0 || !Xk || !W || !b || !cin_channels_ok(N, n_hid, dir0) ||
      (n_hid > 0 && !Xn) || (dir0 < N && (!pooled || pool_off < 0 ||
                                          pool_off + (N - dir0) > pool_ld))) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  if (B == 0) return 0;
  const int nc = cin_nc(N), nu = (m + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CIN(C, U)                                                                        \
  if (nc == C && nu == U)                                                                      \
    return launch_cin_fwd<C, U>(X0, Xk, B, m, H, D, W, b, N, n_hid, dir0, Xn, pooled, pool_off, \
                                pool_ld, st, what);
  MIREC_CIN_FORMS(MIREC_CIN)
#undef MIREC_CIN
  return -1;
}

static int cin_grad_args(const char* what, int64_t B, int32_t m, int32_t H, int32_t D, int32_t N,
                         int32_t n_hid, int32_t dir0, const float* X0, const float* Xk,
                         const float* dXn, const float* g_pooled, int32_t pool_off,
                         int32_t pool_ld, CinGrad* g) {
  if (!mirec_cin_shape_ok(m, H, D, N)) return cin_shape_error(what, m, H, D, N);
  if (B < 0 || !X0 || !Xk || !cin_channels_ok(N, n_hid, dir0) ||
      (dir0 < N && (!g_pooled || pool_off < 0 || pool_off + (N - dir0) > pool_ld))) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  *g = CinGrad{dXn, g_pooled, n_hid, dir0, N, pool_off, pool_ld};
  return 0;
}

extern "C" int mirec_cin_layer_bwd_f32(const float* X0, const float* Xk, int64_t B, int32_t m,
                                       int32_t H, int32_t D, const float* W, int32_t N,
                                       int32_t n_hid, int32_t dir0, const float* dXn,
                                       const float* g_pooled, int32_t pool_off, int32_t pool_ld,
                                       float* dXk, float* dX0, int32_t accumulate, void* stream) {
  const char* what = "mirec_cin_layer_bwd_f32";
  CinGrad g;
  if (cin_grad_args(what, B, m, H, D, N, n_hid, dir0, X0, Xk, dXn, g_pooled, pool_off, pool_ld,
                    &g))
    return -1;
  if (!W || !dX0 || (!dXk && (Xk != X0 || H != m))) {
    set_error("%s: bad arguments (dXk may be NULL only for layer 0, Xk = X0)", what);
    return -1;
  }
  if (B == 0) return 0;
  const int nk = cin_nc(N), nu = (m + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CIN(C, U)                                                                      \
  if (nk == C && nu == U)                                                                    \
    return launch_cin_bwd<C, U>(X0, Xk, B * D, m, H, D, W, g, dXk, dX0, accumulate, st, what);
  MIREC_CIN_FORMS(MIREC_CIN)
#undef MIREC_CIN
  return -1;
}

extern "C" int32_t mirec_cin_wgrad_splits(int64_t B, int32_t m, int32_t H, int32_t D) {
  if (B <= 0 || m < 1 || H < 1 || D < 1) return 0;
  return cin_wgrad_split(B * D, m, H).splits;
}

extern "C" int64_t mirec_cin_wgrad_stride(int32_t N, int32_t K) {
  if (N < 0 || K < 0) return -1;
  return pad4((int64_t)N * K) + pad4(N);
}

extern "C" int mirec_cin_wgrad_f32(const float* X0, const float* Xk, int64_t B, int32_t m,
                                   int32_t H, int32_t D, int32_t N, int32_t n_hid, int32_t dir0,
                                   const float* dXn, const float* g_pooled, int32_t pool_off,
                                   int32_t pool_ld, float* partials, void* stream) {
  const char* what = "mirec_cin_wgrad_f32";
  CinGrad g;
  if (cin_grad_args(what, B, m, H, D, N, n_hid, dir0, X0, Xk, dXn, g_pooled, pool_off, pool_ld,
                    &g))
    return -1;
  if (B <= 0 || !partials) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  const RowSplit sp = cin_wgrad_split(B * D, m, H);
  const int64_t stride = mirec_cin_wgrad_stride(N, H * m);
  const int64_t db_off = pad4((int64_t)N * H * m);
  const int nc = cin_nc(N);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CIN(C, U)                                                                      \
  if (nc == C)                                                                               \
    return launch_cin_wgrad<C>(X0, Xk, B * D, m, H, D, g, sp.rows, sp.splits, partials,      \
                               stride, db_off, st, what);
  MIREC_CIN_TILES(MIREC_CIN, 0)
#undef MIREC_CIN
  return -1;
}
