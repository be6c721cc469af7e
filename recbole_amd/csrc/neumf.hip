// K14 — NeuMF (reference recbole/model/general_recommender/neumf.py).
//
//   logit(u, i) = (w_mf . (U_mf[u] * I_mf[i])) + w_h . MLP([U_mlp[u] | I_mlp[i]]) + b
//
// K14a  the four row gathers of a training batch in one launch: x = [U_mlp[u] | I_mlp[i]]
//       (the MLP input K10 then runs) and z_mf = sum_k w_mf[k] U_mf[u,k] I_mf[i,k].
// K14b  its backward in one launch: the per-row gradients of the four tables (grouped and
//       applied by K2 on the host side) and dw_mf, summed in a fixed order by one block.
// K14c  the pair-MLP full-sort scorer. The first MLP layer is linear in the concatenation,
//       so it splits into a user part A = U_mlp W1u^T + b1 and an item part Bm = I_mlp W1i^T
//       (mirec_neumf_project_f32, once per user batch / once per evaluation) and
//       h1(u, i) = relu(A[u] + Bm[i]). A workgroup takes 32 users and sweeps every item in
//       tiles; a wave takes blocks of 2 users x 16 items = 32 pairs: h1 is formed on the fly
//       as the A operand of layer 2, layers 2..L run on fp32 MFMA (16x16x4, K10's k
//       permutation so both operands load as float4), activations go through the wave's own
//       LDS rows between layers, and the last hidden layer's epilogue folds the head
//       (w_h . h_L) into a 16-lane reduction. The tile's logits land in LDS, get the MF dot
//       and the bias, and are then either stored (scores mode) or scanned by one thread per
//       user into a register top-K behind the pad / history mask (K6's order: score desc,
//       item id asc). No [users x items x anything] tensor exists in HBM.
#include "common.h"
#include "mfma.h"
#include "topk.h"

namespace mirec {

constexpr int kGatherThreads = 256;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// ------------------------------------------------------------------------------- K14a
// One wave per batch row. Ids outside the tables give zero rows.
__global__ __launch_bounds__(kGatherThreads) void neumf_gather_kernel(
    const int64_t* __restrict__ user, const int64_t* __restrict__ item, int64_t B,
    const float* __restrict__ U_mf, const float* __restrict__ I_mf, int dmf,
    const float* __restrict__ w_mf, const float* __restrict__ U_mlp,
    const float* __restrict__ I_mlp, int dm, int64_t n_users, int64_t n_items,
    float* __restrict__ x, float* __restrict__ z_mf) {
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * (kGatherThreads / 64) + (threadIdx.x >> 6);
  if (b >= B) return;
  const int64_t u = user[b], i = item[b];
  const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items;
  if (x) {
    const int v4 = dm / 4;
    for (int f = lane; f < 2 * v4; f += 64) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) v = f < v4 ? ld4(U_mlp + u * dm + 4 * f) : ld4(I_mlp + i * dm + 4 * (f - v4));
      st4(x + b * 2 * dm + 4 * f, v);
    }
  }
  if (z_mf) {
    float acc = 0.f;
    if (U_mf && ok) {
      for (int f = lane; f < dmf / 4; f += 64) {
        const float4 a = ld4(U_mf + u * dmf + 4 * f), c = ld4(I_mf + i * dmf + 4 * f);
        const float4 w = ld4(w_mf + 4 * f);
        acc = fmaf(w.x * a.x, c.x, acc);
        acc = fmaf(w.y * a.y, c.y, acc);
        acc = fmaf(w.z * a.z, c.z, acc);
        acc = fmaf(w.w * a.w, c.w, acc);
      }
    }
    acc = wave_sum(acc);                       // a fixed tree: run to run identical
    if (lane == 0) z_mf[b] = acc;
  }
}

// ------------------------------------------------------------------------------- K14b
// Blocks [0, row_blocks): one wave per batch row writes its gradient rows. The last block
// alone forms dw_mf: thread (slice, float4 column) sums the rows b = slice, slice + S, ...
// in that order, the S slices are then added in slice order — no float atomics.
__global__ __launch_bounds__(kGatherThreads) void neumf_gather_bwd_kernel(
    const int64_t* __restrict__ user, const int64_t* __restrict__ item, int64_t B,
    const float* __restrict__ U_mf, const float* __restrict__ I_mf, int dmf,
    const float* __restrict__ w_mf, const float* __restrict__ g, const float* __restrict__ gx,
    int dm, int64_t n_users, int64_t n_items, float* __restrict__ gU_mf,
    float* __restrict__ gI_mf, float* __restrict__ gU_mlp, float* __restrict__ gI_mlp,
    float* __restrict__ dw_mf, int row_blocks) {
  __shared__ float4 part[kGatherThreads];
  const int lane = threadIdx.x & 63;
  if ((int)blockIdx.x < row_blocks) {
    const int64_t b = (int64_t)blockIdx.x * (kGatherThreads / 64) + (threadIdx.x >> 6);
    if (b >= B) return;
    if (gx) {
      const int v4 = dm / 4;
      for (int f = lane; f < 2 * v4; f += 64) {
        const float4 v = ld4(gx + b * 2 * dm + 4 * f);
        if (f < v4) st4(gU_mlp + b * dm + 4 * f, v);
        else st4(gI_mlp + b * dm + 4 * (f - v4), v);
      }
    }
    if (gU_mf) {
      const int64_t u = user[b], i = item[b];
      const bool ok = u >= 0 && u < n_users && i >= 0 && i < n_items;
      const float gb = g[b];
      for (int f = lane; f < dmf / 4; f += 64) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        if (ok) { a = ld4(U_mf + u * dmf + 4 * f); c = ld4(I_mf + i * dmf + 4 * f); }
        const float4 w = ld4(w_mf + 4 * f);
        const float4 gw = make_float4(gb * w.x, gb * w.y, gb * w.z, gb * w.w);
        st4(gU_mf + b * dmf + 4 * f, make_float4(gw.x * c.x, gw.y * c.y, gw.z * c.z, gw.w * c.w));
        st4(gI_mf + b * dmf + 4 * f, make_float4(gw.x * a.x, gw.y * a.y, gw.z * a.z, gw.w * a.w));
      }
    }
    return;
  }
  if (!dw_mf) return;
  const int v4 = dmf / 4;                        // <= 64 float4 columns (dmf <= 256)
  const int S = kGatherThreads / v4;             // batch slices
  const int col = threadIdx.x % v4, sl = threadIdx.x / v4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (sl < S) {
    for (int64_t b = sl; b < B; b += S) {
      const int64_t u = user[b], i = item[b];
      if (!(u >= 0 && u < n_users && i >= 0 && i < n_items)) continue;
      const float gb = g[b];
      const float4 a = ld4(U_mf + u * dmf + 4 * col), c = ld4(I_mf + i * dmf + 4 * col);
      acc.x = fmaf(gb * a.x, c.x, acc.x);
      acc.y = fmaf(gb * a.y, c.y, acc.y);
      acc.z = fmaf(gb * a.z, c.z, acc.z);
      acc.w = fmaf(gb * a.w, c.w, acc.w);
    }
  }
  part[threadIdx.x] = acc;
  __syncthreads();
  if ((int)threadIdx.x < v4) {
    float4 t = part[threadIdx.x];
    for (int s = 1; s < S; ++s) {
      const float4 p = part[s * v4 + threadIdx.x];
      t.x += p.x; t.y += p.y; t.z += p.z; t.w += p.w;
    }
    st4(dw_mf + 4 * threadIdx.x, t);
  }
}

// --------------------------------------------------------------- first-layer projections
// out[r, h] = bias[h] + sum_k T[row(r), k] W[h, col0 + k] (row(r) = idx[r], or r when idx is
// NULL): A and Bm of K14c. 16 rows per block, staged in LDS; thread -> (row, h).
constexpr int kProjRows = 16;
__global__ __launch_bounds__(256) void neumf_project_kernel(
    const float* __restrict__ T, const int64_t* __restrict__ idx, int64_t n, int64_t n_rows,
    int dm, const float* __restrict__ W, int ldw, int col0, const float* __restrict__ bias,
    int H, float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rows[];          // [16][dm]
  const int64_t r0 = (int64_t)blockIdx.x * kProjRows;
  for (int f = threadIdx.x; f < kProjRows * dm; f += blockDim.x) {
    const int r = f / dm, k = f - r * dm;
    float v = 0.f;
    if (r0 + r < n) {
      const int64_t row = idx ? idx[r0 + r] : r0 + r;
      if (row >= 0 && row < n_rows) v = T[row * dm + k];
    }
    rows[f] = v;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kProjRows * H; e += blockDim.x) {
    const int r = e / H, h = e - r * H;
    if (r0 + r >= n) break;
    const float* w = W + (int64_t)h * ldw + col0;
    float acc = bias ? bias[h] : 0.f;
    for (int k = 0; k < dm; ++k) acc = fmaf(rows[r * dm + k], w[k], acc);
    out[(r0 + r) * H + h] = acc;
  }
}

// ------------------------------------------------------------------------------- K14c
constexpr int kPairTU = 32;           // users per workgroup
constexpr int kPairThreads = 256;     // at most (4 waves); fewer when LDS is short

struct PairCfg {
  int TI;                 // items per tile (multiple of 16)
  int wlds;               // weights of layers 2..L staged in LDS
  int ldH1, ld0, ld1, ldL;
  int oA, oPq, oB, oL, oAct, actStride;   // float offsets into the dynamic LDS
  int oW[4];
};

__device__ __forceinline__ float relu_f(float z) { return z < 0.f ? 0.f : z; }   // NaN passes

// The wave's LDS rows written by some lanes are read by others: order them.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One layer for a wave's 32 pairs (row tile r = user r of the block, 16 items):
// out[32, N] = relu(in[32, K] W^T + bias). ONFLY: in = relu(a_r + b) formed from the
// user rows a0 / a1 and this lane's item row brow; else the wave's LDS rows `in`.
// LAST: the head folded in — part[r][rr] += w_h[c] out[row][c] — instead of a store.
template <bool ONFLY, bool LAST>
__device__ __forceinline__ void pair_layer(const float* W, int ldw, const float* __restrict__ bias,
                                           int K, int N, const float* a0, const float* a1,
                                           const float* brow, const float* in, int ld_in,
                                           float* outp, int ld_out,
                                           const float* __restrict__ w_h, float (&part)[2][4],
                                           int li, int lk) {
  for (int cg = 0; cg < N; cg += 64) {
    floatx4 acc[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[r][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int nj = (N - cg) / 16 < 4 ? (N - cg) / 16 : 4;
    const float* wrow[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = cg + 16 * j + li;
      wrow[j] = W + (int64_t)(c < N ? c : N - 1) * ldw + 4 * lk;
    }
    for (int k = 0; k < K; k += 16) {
      float4 x0, x1;
      if (ONFLY) {
        const float4 bv = ld4(brow + k + 4 * lk);
        const float4 u0 = ld4(a0 + k + 4 * lk), u1 = ld4(a1 + k + 4 * lk);
        x0 = make_float4(relu_f(u0.x + bv.x), relu_f(u0.y + bv.y), relu_f(u0.z + bv.z),
                         relu_f(u0.w + bv.w));
        x1 = make_float4(relu_f(u1.x + bv.x), relu_f(u1.y + bv.y), relu_f(u1.z + bv.z),
                         relu_f(u1.w + bv.w));
      } else {
        x0 = ld4(in + li * ld_in + k + 4 * lk);
        x1 = ld4(in + (16 + li) * ld_in + k + 4 * lk);
      }
      float4 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = ld4(wrow[j] + k);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nj) {                              // wave-uniform
          acc[0][j] = mfma_16x16x4(x0.x, w[j].x, acc[0][j]);
          acc[1][j] = mfma_16x16x4(x1.x, w[j].x, acc[1][j]);
          acc[0][j] = mfma_16x16x4(x0.y, w[j].y, acc[0][j]);
          acc[1][j] = mfma_16x16x4(x1.y, w[j].y, acc[1][j]);
          acc[0][j] = mfma_16x16x4(x0.z, w[j].z, acc[0][j]);
          acc[1][j] = mfma_16x16x4(x1.z, w[j].z, acc[1][j]);
          acc[0][j] = mfma_16x16x4(x0.w, w[j].w, acc[0][j]);
          acc[1][j] = mfma_16x16x4(x1.w, w[j].w, acc[1][j]);
        }
      }
    }
    // epilogue: lane holds rows 4 lk + rr of column c of both row tiles
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < nj) {
        const int c = cg + 16 * j + li;
        const float bc = bias ? bias[c] : 0.f;
        const float wh = LAST ? w_h[c] : 0.f;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) {
            const float z = relu_f(acc[r][j][rr] + bc);
            if (LAST) part[r][rr] = fmaf(wh, z, part[r][rr]);
            else outp[(16 * r + 4 * lk + rr) * ld_out + c] = z;
          }
      }
    }
  }
}

template <int KC, bool SCORES, bool WLDS>
__global__ __launch_bounds__(kPairThreads) void pair_mlp_kernel(
    mirec_pair_mlp m, PairCfg c, const float* __restrict__ A, const float* __restrict__ Pq,
    int64_t nq, const float* __restrict__ Bm, const float* __restrict__ I_mf, int64_t I,
    const int64_t* __restrict__ hist_ptr, const int32_t* __restrict__ hist_cols,
    const int64_t* __restrict__ pos_ptr, const int32_t* __restrict__ pos_cols, int K,
    float* __restrict__ top_scores, int32_t* __restrict__ top_ids,
    uint8_t* __restrict__ pos_flags, float* __restrict__ S) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int lane = tid & 63, wave = tid >> 6, NW = nthr >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int L = m.n_hidden, H1 = m.H[0], dmf = m.dmf, TI = c.TI;
  const int64_t q0 = (int64_t)blockIdx.x * kPairTU;
  float* const sA = lds + c.oA;
  float* const sPq = lds + c.oPq;
  float* const sB = lds + c.oB;
  float* const sL = lds + c.oL;
  float* const act0 = lds + c.oAct + wave * c.actStride;
  float* const act1 = act0 + 32 * c.ld0;

  // once per workgroup: the users' first-layer rows, their MF rows, the weights
  {
    const int v4 = H1 / 4;
    for (int f = tid; f < kPairTU * v4; f += nthr) {
      const int row = f / v4, c4 = f - row * v4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q0 + row < nq) v = ld4(A + (q0 + row) * H1 + 4 * c4);
      st4(sA + row * c.ldH1 + 4 * c4, v);
    }
    const int p4 = dmf / 4;
    for (int f = tid; f < kPairTU * p4; f += nthr) {
      const int row = f / p4, c4 = f - row * p4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q0 + row < nq) v = ld4(Pq + (q0 + row) * dmf + 4 * c4);
      st4(sPq + row * dmf + 4 * c4, v);
    }
    if (WLDS) {
      for (int l = 1; l < L; ++l) {
        const int Kl = m.H[l - 1], w4 = Kl / 4;
        for (int f = tid; f < m.H[l] * w4; f += nthr) {
          const int row = f / w4, c4 = f - row * w4;
          st4(lds + c.oW[l] + row * (Kl + 4) + 4 * c4, ld4(m.W[l] + (int64_t)row * Kl + 4 * c4));
        }
      }
    }
  }

  // per-user state of thread tid < 32: the register top-K and the history cursor
  float ts[KC];
  int ti[KC];
#pragma unroll
  for (int t = 0; t < KC; ++t) { ts[t] = -INFINITY; ti[t] = -1; }
  float thr = -INFINITY;
  const int64_t qu = q0 + tid;
  const bool owner = !SCORES && tid < kPairTU && qu < nq;
  int64_t hcur = 0, hend = 0, hnext = INT64_MAX;
  if (owner && hist_ptr) {
    hcur = hist_ptr[qu];
    hend = hist_ptr[qu + 1];
    if (hcur < hend) hnext = hist_cols[hcur];
  }
  const float bias = m.bias ? m.bias[0] : 0.f;
  const float* __restrict__ w_h = m.w_h;

  for (int64_t base = 0; base < I; base += TI) {
    {                                             // the tile's item rows of Bm
      const int v4 = H1 / 4;
      for (int f = tid; f < TI * v4; f += nthr) {
        const int row = f / v4, c4 = f - row * v4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (base + row < I) v = ld4(Bm + (base + row) * H1 + 4 * c4);
        st4(sB + row * c.ldH1 + 4 * c4, v);
      }
    }
    __syncthreads();
    const int nig = TI / 16, nblk = (kPairTU / 2) * nig;
    for (int blk = wave; blk < nblk; blk += NW) {
      const int up = blk / nig, ig = blk - up * nig;
      float part[2][4];
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) part[r][rr] = 0.f;
      const float* a0 = sA + (2 * up) * c.ldH1;
      const float* a1 = a0 + c.ldH1;
      const float* brow = sB + (16 * ig + li) * c.ldH1;
      for (int l = 1; l < L; ++l) {
        const int Kl = m.H[l - 1], Nl = m.H[l];
        const float* W = WLDS ? (const float*)(lds + c.oW[l]) : m.W[l];
        const int ldw = WLDS ? Kl + 4 : Kl;
        const float* in = l == 2 ? act0 : act1;
        const int ld_in = l == 2 ? c.ld0 : c.ld1;
        float* outp = l == 1 ? act0 : act1;
        const int ld_out = l == 1 ? c.ld0 : c.ld1;
        const bool last = l == L - 1;
        if (l == 1) {
          if (last) pair_layer<true, true>(W, ldw, m.b[l], Kl, Nl, a0, a1, brow, in, ld_in, outp, ld_out, w_h, part, li, lk);
          else pair_layer<true, false>(W, ldw, m.b[l], Kl, Nl, a0, a1, brow, in, ld_in, outp, ld_out, w_h, part, li, lk);
        } else {
          if (last) pair_layer<false, true>(W, ldw, m.b[l], Kl, Nl, a0, a1, brow, in, ld_in, outp, ld_out, w_h, part, li, lk);
          else pair_layer<false, false>(W, ldw, m.b[l], Kl, Nl, a0, a1, brow, in, ld_in, outp, ld_out, w_h, part, li, lk);
        }
        if (!last) wave_lds_sync();
      }
      // the head: sum over the 16 column lanes (a fixed xor tree)
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          float v = part[r][rr];
          v += __shfl_xor(v, 1, 64);
          v += __shfl_xor(v, 2, 64);
          v += __shfl_xor(v, 4, 64);
          v += __shfl_xor(v, 8, 64);
          if (li == 0) sL[(2 * up + r) * c.ldL + 16 * ig + 4 * lk + rr] = v;
        }
    }
    __syncthreads();
    // the MF dot and the bias; scores mode stores the logits
    for (int p = tid; p < kPairTU * TI; p += nthr) {
      const int u = p / TI, i = p - u * TI;
      const int64_t item = base + i;
      if (item >= I) continue;
      float v = sL[u * c.ldL + i] + bias;
      if (dmf) {
        const float* pu = sPq + u * dmf;
        const float* pi = I_mf + item * dmf;
        float acc = 0.f;
        for (int k = 0; k < dmf; k += 4) {
          const float4 a = ld4(pu + k), b = ld4(pi + k);
          acc = fmaf(a.x, b.x, acc);
          acc = fmaf(a.y, b.y, acc);
          acc = fmaf(a.z, b.z, acc);
          acc = fmaf(a.w, b.w, acc);
        }
        v += acc;
      }
      if (SCORES) {
        if (q0 + u < nq) S[(q0 + u) * I + item] = v;
      } else {
        sL[u * c.ldL + i] = v;
      }
    }
    if (!SCORES) {
      __syncthreads();
      if (owner) {                                // increasing item id: strict '>' keeps id asc
        const int lim = (int)(I - base < TI ? I - base : TI);
        for (int i = 0; i < lim; ++i) {
          const int64_t item = base + i;
          const float v = sL[tid * c.ldL + i];
          while (hnext < item) {
            ++hcur;
            hnext = hcur < hend ? (int64_t)hist_cols[hcur] : INT64_MAX;
          }
          if (item != 0 && hnext != item && v > thr) {
            topk_insert<KC>(ts, ti, v, (int)item);
            thr = ts[KC - 1];
          }
        }
      }
    }
  }

  if (owner) {
    const int64_t p0 = pos_ptr ? pos_ptr[qu] : 0;
    const int64_t p1 = pos_ptr ? pos_ptr[qu + 1] : 0;
#pragma unroll
    for (int t = 0; t < KC; ++t) {
      if (t < K) {
        const int64_t o = qu * K + t;
        if (top_scores) top_scores[o] = ts[t];
        if (top_ids) top_ids[o] = ti[t];
        if (pos_flags)
          pos_flags[o] = (ti[t] >= 0 && sorted_contains(pos_cols, p0, p1, ti[t])) ? 1 : 0;
      }
    }
  }
}

constexpr size_t kPairLdsMax = 160 * 1024;    // LDS of a gfx950 CU

// The LDS layout for (TI, waves, weights in LDS); returns its bytes.
static size_t pair_layout(const mirec_pair_mlp& m, int TI, int NW, int wlds, PairCfg* c) {
  const int L = m.n_hidden;
  auto r4 = [](int x) { return (x + 3) / 4 * 4; };
  memset(c, 0, sizeof(*c));
  c->TI = TI;
  c->wlds = wlds;
  c->ldH1 = m.H[0] + 4;
  c->ld0 = L >= 3 ? m.H[1] + 4 : 0;
  c->ld1 = L >= 4 ? m.H[2] + 4 : 0;
  c->ldL = TI + 1;
  int o = 0;
  c->oA = o; o += kPairTU * c->ldH1;
  c->oPq = o; o += r4(kPairTU * m.dmf);
  c->oB = o; o += TI * c->ldH1;
  c->oL = o; o += r4(kPairTU * c->ldL);
  c->actStride = 32 * (c->ld0 + c->ld1);
  c->oAct = o; o += NW * c->actStride;
  for (int l = 1; l < L; ++l) {
    c->oW[l] = o;
    if (wlds) o += m.H[l] * (m.H[l - 1] + 4);
  }
  return (size_t)o * sizeof(float);
}

static int pair_check(const mirec_pair_mlp* m, const char* what) {
  bool ok = m && m->n_hidden >= 2 && m->n_hidden <= 4 && m->w_h && m->dmf >= 0 &&
            m->dmf <= 128 && m->dmf % 4 == 0;
  if (ok)
    for (int l = 0; l < m->n_hidden; ++l) {
      ok = ok && m->H[l] >= 16 && m->H[l] <= 256 && m->H[l] % 16 == 0;
      if (l >= 1) ok = ok && m->W[l] && ((uintptr_t)m->W[l] % 16 == 0);
    }
  if (!ok)
    set_error("%s: bad descriptor (2..4 hidden layers, widths multiples of 16 in 16..256, "
              "dmf a multiple of 4 up to 128, 16-B aligned weights)", what);
  return ok ? 0 : -1;
}

template <int KC, bool SCORES, bool WLDS>
static int pair_launch(const mirec_pair_mlp& m, const PairCfg& c, size_t shm, int NW,
                       const float* A, const float* Pq, int64_t nq, const float* Bm,
                       const float* I_mf, int64_t I, const int64_t* hist_ptr,
                       const int32_t* hist_cols, const int64_t* pos_ptr, const int32_t* pos_cols,
                       int K, float* top_scores, int32_t* top_ids, uint8_t* pos_flags, float* S,
                       hipStream_t st) {
  auto kern = pair_mlp_kernel<KC, SCORES, WLDS>;
  // shm varies with the layer widths: allow the most any descriptor is given
  static int cache[kMaxDev] = {};
  const int rc = prepare_launch(kern, 64 * NW, kPairLdsMax, cache, nullptr,
                                "mirec_pair_mlp: LDS size attribute");
  if (rc) return rc;
  hipLaunchKernelGGL(kern, dim3((unsigned)((nq + kPairTU - 1) / kPairTU)), dim3(64 * NW), shm, st,
                     m, c, A, Pq, nq, Bm, I_mf, I, hist_ptr, hist_cols, pos_ptr, pos_cols, K,
                     top_scores, top_ids, pos_flags, S);
  return launch_status("mirec_pair_mlp");
}

}  // namespace mirec

using namespace mirec;

extern "C" int mirec_neumf_gather_f32(const int64_t* user, const int64_t* item, int64_t B,
                                      const float* U_mf, const float* I_mf, int32_t dmf,
                                      const float* w_mf, const float* U_mlp, const float* I_mlp,
                                      int32_t dm, int64_t n_users, int64_t n_items, float* x,
                                      float* z_mf, void* stream) {
  if (B == 0) return 0;
  const bool mf = U_mf != nullptr, mlp = x != nullptr;
  if (!user || !item || B < 0 || n_users <= 0 || n_items <= 0 || !z_mf ||
      (mf && (!I_mf || !w_mf || dmf < 4 || dmf % 4 || dmf > 256)) ||
      (mlp && (!U_mlp || !I_mlp || dm < 4 || dm % 4))) {
    set_error("mirec_neumf_gather_f32: bad arguments (widths multiples of 4, dmf <= 256)");
    return -1;
  }
  const int rpb = kGatherThreads / 64;
  hipLaunchKernelGGL(neumf_gather_kernel, dim3((unsigned)((B + rpb - 1) / rpb)),
                     dim3(kGatherThreads), 0, (hipStream_t)stream, user, item, B, U_mf, I_mf,
                     (int)dmf, w_mf, U_mlp, I_mlp, (int)dm, n_users, n_items, x, z_mf);
  return launch_status("mirec_neumf_gather_f32");
}

extern "C" int mirec_neumf_gather_bwd_f32(const int64_t* user, const int64_t* item, int64_t B,
                                          const float* U_mf, const float* I_mf, int32_t dmf,
                                          const float* w_mf, const float* g, const float* gx,
                                          int32_t dm, int64_t n_users, int64_t n_items,
                                          float* gU_mf, float* gI_mf, float* gU_mlp,
                                          float* gI_mlp, float* dw_mf, void* stream) {
  if (B == 0) return 0;
  const bool mf = gU_mf != nullptr, mlp = gx != nullptr;
  if (!user || !item || B < 0 || n_users <= 0 || n_items <= 0 ||
      (mf && (!U_mf || !I_mf || !w_mf || !g || !gI_mf || !dw_mf || dmf < 4 || dmf % 4 ||
              dmf > 256)) ||
      (mlp && (!gU_mlp || !gI_mlp || dm < 4 || dm % 4))) {
    set_error("mirec_neumf_gather_bwd_f32: bad arguments (widths multiples of 4, dmf <= 256)");
    return -1;
  }
  const int rpb = kGatherThreads / 64;
  const int row_blocks = (int)((B + rpb - 1) / rpb);
  hipLaunchKernelGGL(neumf_gather_bwd_kernel, dim3((unsigned)(row_blocks + (mf ? 1 : 0))),
                     dim3(kGatherThreads), 0, (hipStream_t)stream, user, item, B, U_mf, I_mf,
                     (int)dmf, w_mf, g, gx, (int)dm, n_users, n_items, gU_mf, gI_mf, gU_mlp,
                     gI_mlp, mf ? dw_mf : nullptr, row_blocks);
  return launch_status("mirec_neumf_gather_bwd_f32");
}

extern "C" int mirec_neumf_project_f32(const float* T, const int64_t* idx, int64_t n,
                                       int64_t n_rows, int32_t dm, const float* W, int32_t ldw,
                                       int32_t col0, const float* bias, int32_t H, float* out,
                                       void* stream) {
  if (n == 0) return 0;
  if (!T || !W || !out || n < 0 || n_rows <= 0 || dm < 1 || dm > 1024 || H < 1 || col0 < 0 ||
      ldw < col0 + dm) {
    set_error("mirec_neumf_project_f32: bad arguments (1 <= dm <= 1024, ldw >= col0 + dm)");
    return -1;
  }
  hipLaunchKernelGGL(neumf_project_kernel, dim3((unsigned)((n + kProjRows - 1) / kProjRows)),
                     dim3(256), (size_t)kProjRows * dm * sizeof(float), (hipStream_t)stream, T, idx,
                     n, n_rows, (int)dm, W, (int)ldw, (int)col0, bias, (int)H, out);
  return launch_status("mirec_neumf_project_f32");
}

extern "C" int mirec_pair_mlp_supported(const mirec_pair_mlp* m) {
  if (pair_check(m, "mirec_pair_mlp_supported")) return 0;
  PairCfg c;
  return pair_layout(*m, 16, 1, 0, &c) <= kPairLdsMax ? 1 : 0;
}

extern "C" int mirec_pair_mlp_f32(const mirec_pair_mlp* mlp, const float* A, const float* Pq,
                                  int64_t nq, const float* Bm, const float* I_mf, int64_t I,
                                  const int64_t* hist_ptr, const int32_t* hist_cols,
                                  const int64_t* pos_ptr, const int32_t* pos_cols, int32_t K,
                                  float* top_scores, int32_t* top_ids, uint8_t* pos_flags,
                                  float* scores, void* stream) {
  if (nq == 0) return 0;
  if (pair_check(mlp, "mirec_pair_mlp_f32")) return -1;
  const mirec_pair_mlp& m = *mlp;
  const bool sc = scores != nullptr;
  if (!A || !Bm || nq < 0 || I <= 0 || I > INT32_MAX || (m.dmf && (!Pq || !I_mf)) ||
      (!sc && (K < 1 || K > 50)) || (hist_ptr && !hist_cols) || (pos_ptr && !pos_cols) ||
      (pos_flags && !pos_ptr) || ((uintptr_t)A % 16) || ((uintptr_t)Bm % 16) ||
      (m.dmf && (((uintptr_t)Pq % 16) || ((uintptr_t)I_mf % 16)))) {
    set_error("mirec_pair_mlp_f32: bad arguments (1 <= K <= 50, I <= 2^31 - 1, 16-B aligned rows)");
    return -1;
  }
  // the widest configuration whose LDS fits: weights in LDS, 64-item tiles, 4 waves first
  static const int cand[][3] = {{1, 64, 4}, {1, 32, 4}, {0, 64, 4}, {0, 32, 4},
                                {0, 16, 4}, {0, 16, 2}, {0, 16, 1}};
  PairCfg c;
  size_t shm = 0;
  int NW = 0, wl = 0;
  for (const auto& k : cand) {
    shm = pair_layout(m, k[1], k[2], k[0], &c);
    if (shm <= kPairLdsMax) { wl = k[0]; NW = k[2]; break; }
  }
  if (!NW) {
    set_error("mirec_pair_mlp_f32: the layer widths need %zu B of LDS", shm);
    return -1;
  }
  hipStream_t st = (hipStream_t)stream;
#define MIREC_PAIR(KK, SS, WW)                                                                  \
  return pair_launch<KK, SS, WW>(m, c, shm, NW, A, Pq, nq, Bm, I_mf, I, hist_ptr, hist_cols,    \
                                 pos_ptr, pos_cols, K, top_scores, top_ids, pos_flags, scores, st)
  if (sc) {
    if (wl) MIREC_PAIR(1, true, true);
    MIREC_PAIR(1, true, false);
  }
  if (K <= 10) {
    if (wl) MIREC_PAIR(10, false, true);
    MIREC_PAIR(10, false, false);
  }
  if (K <= 20) {
    if (wl) MIREC_PAIR(20, false, true);
    MIREC_PAIR(20, false, false);
  }
  if (wl) MIREC_PAIR(50, false, true);
  MIREC_PAIR(50, false, false);
#undef MIREC_PAIR
}
