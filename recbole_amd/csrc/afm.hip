// K20 — AFM's pairwise-attention layer (reference afm.py:55-99, layers.py AttLayer) on fp32
// MFMA. Per sample, with field rows e_0 .. e_{F-1} [d], pairs p = (i, j), i < j, W [A, d],
// h [A] and pv [d]:
//   z_p = e_i * e_j      u_p = W z_p      s_p = h . relu(u_p)      alpha = softmax_p(s)
//   v = sum_p alpha_p z_p                 y = dropout(v) . pv
// The reference keeps four [B, P, d] and three [B, P, A] tensors (P = F (F - 1) / 2) for
// autograd. Here a workgroup owns whole samples: the sample's F rows go to LDS once, z is
// formed in registers from two LDS rows, W sits zero-padded in LDS for the kernel's life, and
// nothing of size B x P exists in either pass.
//
// Slabs. The pairs of a sample are walked in slabs of 16 with ONE left field: slab (i, j0)
// holds the pairs (i, j0 + q), q < min(16, F - j0), for j0 = i + 1, i + 17, ... (F = 39: 66
// slabs for 741 pairs, against 47 if the pairs were packed; the last slab of a field is
// ragged). That costs MFMA rows but makes the backward's field sums plain: in a slab the
// right fields j are distinct and the left field is one.
//
// Operand layout. The score product runs transposed, C[unit][pair] = W z^T: lane (li, lk)
// supplies W[16c + li][k] as the MFMA's A operand (from LDS) and z[pair li][k] as B, with
// k = 16u + 4lk + {x, y, z, w}, so acc[c][r] = u[unit 16c + 4lk + r][pair li]. The pair sits
// on the lane: s_p, alpha_p and ds_p are per-lane scalars (two shuffles over lk finish a dot
// over the units), and du_p = ds_p h [u_p > 0] is, register for register, the B operand of
// the second product dz^T = W^T du^T (the contracted unit index may be walked in any order as
// long as both operands agree), whose result dz[col 16u + 4lk + r][pair li] lines up with the
// float4s of e_i and e_j the lane already holds. mfma.h's slab product puts the slab row on
// (lk, register) and the weight column on the lane; that is the layout the weight gradient
// dW += du^T z wants (contraction over the pairs), so K20b runs it as well — the same k order,
// hence the same bits of u — and takes ds_p for its four rows from the lanes that own them.
//
//   K20a afm_fwd_kernel  256 threads; waves take slabs w, w + 4, ...; the scores go to LDS
//                        (at most 2,496 floats: an exact two-pass softmax with no rescaling,
//                        and re-forming z for the pooling is one multiply an element, cheaper
//                        than a second MFMA pass or an online softmax's rescaled
//                        accumulators); max and sum over the slabs in a fixed order; the
//                        pooling by (column, part) threads over the pairs, parts added in
//                        order; dropout (drop.h, element b d + column) and the dot with pv
//                        by the first wave. Saved: v [d] before dropout, the max and the sum.
//   K20b afm_bwd_kernel  WV = 16, 8 or 4 waves (the shape decides: launch_afm_bwd_waves), a
//                        workgroup per split of the rows. Per slab: u, s,
//                        alpha recomputed; t = gv . z, ds = alpha (t - c); dz^T by MFMA;
//                        de_j += dz * e_i goes to the wave's own [F][16 NU] LDS copy (distinct
//                        j in a slab), de_i += sum over the slab's lanes of dz * e_j (a DPP
//                        row sum) likewise; after the sample's slabs the WV copies are
//                        added in wave order and dX is written once. dW accumulates in MFMA
//                        registers over the split's samples, dh and dpv in lane registers;
//                        the waves are added in order and split s stores [dW | dh | dpv];
//                        mirec_linear_grad_finish_f32 adds the splits in order.
//
// Every sum has an order fixed by (B, F, d, A): the MFMA k order, the lanes' trees, a wave's
// slabs in order, the waves in order, a split's samples in order, the splits in order. No
// float atomics.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch in any built
// form), NU = ceil(d / 16), NC = ceil(A / 16): K20a 56 - 108 VGPRs + 4 NC AGPRs, dynamic LDS
// <= 47 KB. K20b at 16 waves 107 / 119 / 127 VGPRs (NU NC <= 2; the other forms would spill 24 to
// 556 bytes a lane into scratch at 128 registers), at 8 waves 115 - 231 (NU = NC = 4 would spill
// 40 bytes), at 4 waves 121 - 183 + 8 - 88 AGPRs; dynamic LDS <= 128 KB (102 KB at the widest
// shape, 45 KB at F = 39, d = 16, A = 25).
#include "common.h"
#include "drop.h"
#include "mfma.h"
#include "rowsplit.h"

#include <algorithm>

namespace mirec {

constexpr int kAfmThreads = 256;
constexpr int kAfmWaves = kAfmThreads / 64;
constexpr int kAfmMaxSplits = 32;
constexpr int kAfmMaxF = 64, kAfmMaxD = 64, kAfmMaxA = 64;

// slabs of a sample: sum over i of ceil((F - 1 - i) / 16)
static inline int afm_slabs(int F) {
  int n = 0;
  for (int i = 0; i + 1 < F; ++i) n += (F - 1 - i + 15) / 16;
  return n;
}

// the sum of x over the 16 lanes of a DPP row (fixed lk), in every lane of the row
__device__ __forceinline__ float afm_row16_sum(float x) {
#define MIREC_DPP_ADD(ctrl)                                                                   \
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, false))
  MIREC_DPP_ADD(0xb1);     // quad_perm:[1,0,3,2]
  MIREC_DPP_ADD(0x4e);     // quad_perm:[2,3,0,1]
  MIREC_DPP_ADD(0x124);    // row_ror:4
  MIREC_DPP_ADD(0x128);    // row_ror:8
#undef MIREC_DPP_ADD
  return x;
}

// the sum over the four lk of a lane column (fixed li), the same bits in all four
__device__ __forceinline__ float afm_lk_sum(float x) {
  x += __shfl_xor(x, 16, 64);
  x += __shfl_xor(x, 32, 64);
  return x;
}

__device__ __forceinline__ float afm_wave_sum(float x) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__device__ __forceinline__ float afm_wave_max(float x) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
  return x;
}

// LDS every K20 kernel starts with: W [16 NC][KP] and h [16 NC] zero-padded, pv [16 NU], the
// slab table (i | j0 << 8 | count << 16)
template <int NU, int NC>
struct AfmLds {
  static constexpr int DP = 16 * NU, AP = 16 * NC, XS = DP + 4, KP = DP + 4;
  static constexpr int oW = 0, oH = oW + AP * KP, oPv = oH + AP, oGv = oPv + DP,
                       oRed = oGv + DP, oSlab = oRed + 16;
  __host__ __device__ static int oX(int nsl) { return oSlab + (nsl + 3) / 4 * 4; }
  __host__ __device__ static int end_x(int F, int nsl) { return oX(nsl) + F * XS; }
};

template <int NU, int NC, int TH>
__device__ __forceinline__ void afm_stage_weights(float* smem, const float* __restrict__ W,
                                                  const float* __restrict__ h,
                                                  const float* __restrict__ pv, int F, int d,
                                                  int A) {
  using L = AfmLds<NU, NC>;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < L::AP * L::KP; idx += TH) {
    const int a = idx / L::KP, k = idx - a * L::KP;
    smem[L::oW + idx] = (a < A && k < d) ? W[a * d + k] : 0.f;
  }
  for (int idx = tid; idx < L::AP; idx += TH) smem[L::oH + idx] = idx < A ? h[idx] : 0.f;
  for (int idx = tid; idx < L::DP; idx += TH) smem[L::oPv + idx] = idx < d ? pv[idx] : 0.f;
  if (tid == 0) {
    int* slab = reinterpret_cast<int*>(smem + L::oSlab);
    int n = 0;
    for (int i = 0; i + 1 < F; ++i)
      for (int j0 = i + 1; j0 < F; j0 += 16) slab[n++] = i | (j0 << 8) | (min(16, F - j0) << 16);
  }
}

// a sample's rows, zero-padded to 16 NU columns
template <int NU, int TH>
__device__ __forceinline__ void afm_stage_rows(float* sX, const float* __restrict__ Xb, int F,
                                               int d) {
  constexpr int DP = 16 * NU, XS = DP + 4;
  for (int idx = threadIdx.x; idx < F * DP; idx += TH) {
    const int f = idx / DP, k = idx - f * DP;
    const float v = Xb[f * d + (k < d ? k : d - 1)];
    sX[f * XS + k] = k < d ? v : 0.f;
  }
}

// The transposed score product of the slab (i, j): ei, ej, z = ei * ej (floats 16u + 4lk ..
// +3 of the lane's pair) and acc[c][r] = u[unit 16c + 4lk + r][pair li]. Per accumulator the
// order is u ascending, then x, y, z, w: mfma_slab's order.
template <int NU, int NC>
__device__ __forceinline__ void afm_slab_u(const float* sX, const float* sW, int i, int j, int li,
                                           int lk, float4 (&ei)[NU], float4 (&ej)[NU],
                                           float4 (&z)[NU], floatx4 (&acc)[NC]) {
  constexpr int XS = 16 * NU + 4, KP = XS;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    ei[u] = load_float4(&sX[i * XS + 16 * u + 4 * lk]);
    ej[u] = load_float4(&sX[j * XS + 16 * u + 4 * lk]);
    z[u] = make_float4(ei[u].x * ej[u].x, ei[u].y * ej[u].y, ei[u].z * ej[u].z, ei[u].w * ej[u].w);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    float4 wv[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) wv[c] = load_float4(&sW[(16 * c + li) * KP + 16 * u + 4 * lk]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_16x16x4(wv[c].x, z[u].x, acc[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_16x16x4(wv[c].y, z[u].y, acc[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_16x16x4(wv[c].z, z[u].z, acc[c]);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = mfma_16x16x4(wv[c].w, z[u].w, acc[c]);
  }
}

// s_p = h . relu(u_p) of the lane's pair (the same bits in the four lanes of the pair)
template <int NC>
__device__ __forceinline__ float afm_score(const floatx4 (&acc)[NC], const float4 (&hv)[NC]) {
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    s = fmaf(hv[c].x, fmaxf(acc[c][0], 0.f), s);
    s = fmaf(hv[c].y, fmaxf(acc[c][1], 0.f), s);
    s = fmaf(hv[c].z, fmaxf(acc[c][2], 0.f), s);
    s = fmaf(hv[c].w, fmaxf(acc[c][3], 0.f), s);
  }
  return afm_lk_sum(s);
}

// ---------------------------------------------------------------- K20a
template <int NU, int NC>
__global__ __launch_bounds__(kAfmThreads) void afm_fwd_kernel(
    const float* __restrict__ X, int64_t B, int F, int d, const float* __restrict__ W,
    const float* __restrict__ h, int A, const float* __restrict__ pv, float* __restrict__ y,
    float* __restrict__ V, float* __restrict__ ML, int nsl, int drop, const DropSite dr) {
  using L = AfmLds<NU, NC>;
  constexpr int DP = L::DP, XS = L::XS, NPART = kAfmThreads / DP;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const float* sW = smem + L::oW;
  float* sRed = smem + L::oRed;
  const int* sSlab = reinterpret_cast<const int*>(smem + L::oSlab);
  float* sX = smem + L::oX(nsl);
  float* sS = smem + L::end_x(F, nsl);          // [16 nsl] scores, then exp(s - max)
  float* sPool = sS + 16 * nsl;                 // [NPART][DP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;

  afm_stage_weights<NU, NC, kAfmThreads>(smem, W, h, pv, F, d, A);
  uint64_t key = 0;
  if (drop) {
    const int64_t cv = dr.counter[0];
    if (blockIdx.x == 0 && tid == 0) dr.drawn[0] = cv;
    key = drop_key(dr.seed, cv);
  }
  __syncthreads();
  float4 hv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) hv[c] = load_float4(&smem[L::oH + 16 * c + 4 * lk]);
  const int n_s = 16 * nsl;

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    afm_stage_rows<NU, kAfmThreads>(sX, X + b * F * d, F, d);
    __syncthreads();
    for (int sl = w; sl < nsl; sl += kAfmWaves) {
      const int sd = sSlab[sl], i = sd & 255, j0 = (sd >> 8) & 255, cnt = sd >> 16;
      const bool valid = li < cnt;
      const int j = valid ? j0 + li : F - 1;
      float4 ei[NU], ej[NU], z[NU];
      floatx4 acc[NC];
      afm_slab_u<NU, NC>(sX, sW, i, j, li, lk, ei, ej, z, acc);
      const float s = afm_score<NC>(acc, hv);
      if (lk == 0) sS[16 * sl + li] = valid ? s : -INFINITY;
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int idx = tid; idx < n_s; idx += kAfmThreads) mx = fmaxf(mx, sS[idx]);
    mx = afm_wave_max(mx);
    if (lane == 0) sRed[w] = mx;
    __syncthreads();
    const float m = fmaxf(fmaxf(sRed[0], sRed[1]), fmaxf(sRed[2], sRed[3]));
    float sum = 0.f;
    for (int idx = tid; idx < n_s; idx += kAfmThreads) {
      const float e = expf(sS[idx] - m);
      sS[idx] = e;
      sum += e;
    }
    sum = afm_wave_sum(sum);
    if (lane == 0) sRed[4 + w] = sum;
    __syncthreads();
    const float l = ((sRed[4] + sRed[5]) + sRed[6]) + sRed[7];
    // pooling: thread (column, part) over the pairs part, part + NPART, ...
    {
      const int col = tid % DP, part = tid / DP;       // DP = 48: threads 240 .. 255 idle
      float a = 0.f;
      for (int idx = part; idx < n_s && part < NPART; idx += NPART) {
        const int sd = sSlab[idx >> 4], q = idx & 15;
        const int i = sd & 255, j0 = (sd >> 8) & 255, cnt = sd >> 16;
        if (q < cnt) a = fmaf(sS[idx], sX[i * XS + col] * sX[(j0 + q) * XS + col], a);
      }
      if (part < NPART) sPool[part * DP + col] = a;
    }
    __syncthreads();
    if (w == 0) {
      float v = 0.f, term = 0.f;
      if (lane < DP) {
#pragma unroll
        for (int p = 0; p < NPART; ++p) v += sPool[p * DP + lane];
        v = v / l;
      }
      if (lane < d) {
        V[b * d + lane] = v;
        float vd = v;
        if (drop) vd = drop_keep(key, (uint64_t)b * d + lane, dr.thr) ? v * dr.scale : 0.f;
        term = vd * smem[L::oPv + lane];
      }
      term = afm_wave_sum(term);
      if (lane == 0) {
        y[b] = term;
        ML[2 * b] = m;
        ML[2 * b + 1] = l;
      }
    }
    __syncthreads();                      // sX, sS, sRed and sPool are reused by the next sample
  }
}

// ---------------------------------------------------------------- K20b
template <int NU, int NC, int WV>
__global__ __launch_bounds__(64 * WV) void afm_bwd_kernel(
    const float* __restrict__ X, int64_t B, int F, int d, const float* __restrict__ W,
    const float* __restrict__ h, int A, const float* __restrict__ pv, const float* __restrict__ V,
    const float* __restrict__ ML, const float* __restrict__ gy, float* __restrict__ dX,
    float* __restrict__ partials, int64_t stride, int64_t rows, int splits, int nsl, int big,
    int drop, const DropSite dr) {
  using L = AfmLds<NU, NC>;
  constexpr int DP = L::DP, XS = L::XS, KP = L::KP, TH = 64 * WV;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const float* sW = smem + L::oW;
  const float* sH = smem + L::oH;
  float* sGv = smem + L::oGv;
  float* sRed = smem + L::oRed;
  const int* sSlab = reinterpret_cast<const int*>(smem + L::oSlab);
  float* sX = smem + L::oX(nsl);
  float* sAcc = smem + L::end_x(F, nsl);        // [waves][big]: dX copies, then the dW copies
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  float* sMine = sAcc + w * big;                // this wave's copy

  afm_stage_weights<NU, NC, TH>(smem, W, h, pv, F, d, A);
  uint64_t key = 0;
  if (drop) {
    const int64_t cv = dr.drawn[0];
    if (blockIdx.x == 0 && tid == 0) dr.counter[0] = cv + 1;
    key = drop_key(dr.seed, cv);
  }
  __syncthreads();
  float4 hv[NC];
  float hc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    hv[c] = load_float4(&smem[L::oH + 16 * c + 4 * lk]);
    hc[c] = sH[16 * c + li];
  }

  for (int s = blockIdx.x; s < splits; s += gridDim.x) {
    const int64_t r0 = (int64_t)s * rows, r1 = std::min<int64_t>(r0 + rows, B);
    floatx4 dWacc[NC][NU];
    float dhacc[NC], dpvacc = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      dhacc[c] = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) dWacc[c][u] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

    for (int64_t b = r0; b < r1; ++b) {
      afm_stage_rows<NU, TH>(sX, X + b * F * d, F, d);
      for (int idx = tid; idx < WV * big; idx += TH) sAcc[idx] = 0.f;
      const float gyb = gy[b], m = ML[2 * b], l = ML[2 * b + 1];
      if (w == 0) {
        float gvk = 0.f, vk = 0.f;
        if (lane < d) {
          float kf = 1.f;
          if (drop) kf = drop_keep(key, (uint64_t)b * d + lane, dr.thr) ? dr.scale : 0.f;
          vk = V[b * d + lane];
          gvk = gyb * (kf * smem[L::oPv + lane]);
          dpvacc += gyb * (kf * vk);
        }
        if (lane < DP) sGv[lane] = gvk;
        const float c = afm_wave_sum(gvk * vk);
        if (lane == 0) sRed[0] = c;
      }
      __syncthreads();
      const float cdot = sRed[0];
      float4 gv[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) gv[u] = load_float4(&sGv[16 * u + 4 * lk]);

      for (int sl = w; sl < nsl; sl += WV) {
        const int sd = sSlab[sl], i = sd & 255, j0 = (sd >> 8) & 255, cnt = sd >> 16;
        const bool valid = li < cnt;
        const int j = valid ? j0 + li : F - 1;
        float4 ei[NU], ej[NU], z[NU];
        floatx4 acc[NC];
        afm_slab_u<NU, NC>(sX, sW, i, j, li, lk, ei, ej, z, acc);
        const float sc = afm_score<NC>(acc, hv);
        const float alpha = valid ? expf(sc - m) / l : 0.f;
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          t = fmaf(z[u].x, gv[u].x, t);
          t = fmaf(z[u].y, gv[u].y, t);
          t = fmaf(z[u].z, gv[u].z, t);
          t = fmaf(z[u].w, gv[u].w, t);
        }
        t = afm_lk_sum(t);
        const float ds = alpha * (t - cdot);

        // dz^T = W^T du^T: A = W[unit 16c + 4lk + r][col 16u + li] (LDS), B = du (registers)
        floatx4 dz[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) dz[u] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float hq[4] = {hv[c].x, hv[c].y, hv[c].z, hv[c].w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float du = acc[c][r] > 0.f ? ds * hq[r] : 0.f;
            float wa[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) wa[u] = sW[(16 * c + 4 * lk + r) * KP + 16 * u + li];
#pragma unroll
            for (int u = 0; u < NU; ++u) dz[u] = mfma_16x16x4(wa[u], du, dz[u]);
          }
        }
        // de_j += dz * e_i (distinct j over the slab's lanes); de_i += row sum of dz * e_j
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const float g0 = fmaf(alpha, gv[u].x, dz[u][0]), g1 = fmaf(alpha, gv[u].y, dz[u][1]);
          const float g2 = fmaf(alpha, gv[u].z, dz[u][2]), g3 = fmaf(alpha, gv[u].w, dz[u][3]);
          if (valid) {
            float4* pj = reinterpret_cast<float4*>(&sMine[j * DP + 16 * u + 4 * lk]);
            float4 o = *pj;
            o.x += g0 * ei[u].x;
            o.y += g1 * ei[u].y;
            o.z += g2 * ei[u].z;
            o.w += g3 * ei[u].w;
            *pj = o;
          }
          const float c0 = afm_row16_sum(valid ? g0 * ej[u].x : 0.f);
          const float c1 = afm_row16_sum(valid ? g1 * ej[u].y : 0.f);
          const float c2 = afm_row16_sum(valid ? g2 * ej[u].z : 0.f);
          const float c3 = afm_row16_sum(valid ? g3 * ej[u].w : 0.f);
          if (li == 0) {
            float4* pi = reinterpret_cast<float4*>(&sMine[i * DP + 16 * u + 4 * lk]);
            float4 o = *pi;
            o.x += c0;
            o.y += c1;
            o.z += c2;
            o.w += c3;
            *pi = o;
          }
        }
        __builtin_amdgcn_wave_barrier();   // the wave's next slab reads what other lanes stored

        // the weight gradient's layout: acc1[c][r] = u[pair 4lk + r][unit 16c + li]
        floatx4 acc1[NC];
        mfma_slab<NU, NC, KP>(z, sW, li, lk, acc1);
        float dsr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) dsr[r] = __shfl(ds, 4 * lk + r, 64);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int jr = std::min(j0 + 4 * lk + r, F - 1);     // past the slab: ds = 0
          float bz[NU], a1[NC];
#pragma unroll
          for (int u = 0; u < NU; ++u)
            bz[u] = sX[i * XS + 16 * u + li] * sX[jr * XS + 16 * u + li];
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            a1[c] = acc1[c][r] > 0.f ? dsr[r] * hc[c] : 0.f;
            dhacc[c] = fmaf(dsr[r], fmaxf(acc1[c][r], 0.f), dhacc[c]);
          }
#pragma unroll
          for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int u = 0; u < NU; ++u) dWacc[c][u] = mfma_16x16x4(a1[c], bz[u], dWacc[c][u]);
        }
      }
      __syncthreads();
      // dX[b]: the waves' copies in wave order, written once
      float* dXb = dX + b * F * d;
      for (int idx = tid; idx < F * d; idx += TH) {
        const int f = idx / d, k = idx - f * d;
        float a = sAcc[f * DP + k];
#pragma unroll
        for (int v = 1; v < WV; ++v) a += sAcc[v * big + f * DP + k];
        dXb[idx] = a;
      }
      __syncthreads();
    }

    // the split's sums: dWacc[c][u][q] = dW[unit 16c + 4lk + q][col 16u + li]
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          sMine[(16 * c + 4 * lk + q) * DP + 16 * u + li] = dWacc[c][u][q];
    __syncthreads();
    float* P = partials + (int64_t)s * stride;
    for (int idx = tid; idx < A * d; idx += TH) {
      const int a = idx / d, k = idx - a * d;
      float v = sAcc[a * DP + k];
#pragma unroll
      for (int q = 1; q < WV; ++q) v += sAcc[q * big + a * DP + k];
      P[idx] = v;
    }
    __syncthreads();
    // dh[unit 16c + li]: the four lk of a lane column, then the waves in order
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const float v = afm_lk_sum(dhacc[c]);
      if (lk == 0) sMine[16 * c + li] = v;
    }
    __syncthreads();
    if (tid < A) {
      float v = sAcc[tid];
#pragma unroll
      for (int q = 1; q < WV; ++q) v += sAcc[q * big + tid];
      P[A * d + tid] = v;
    }
    if (tid < d) P[A * d + A + tid] = dpvacc;        // wave 0's lanes own the columns
    for (int64_t idx = (int64_t)A * d + A + d + tid; idx < stride; idx += TH) P[idx] = 0.f;
    __syncthreads();                                  // sAcc is zeroed by the next split
  }
}

// ---------------------------------------------------------------- host side
// mirec_afm_grid_cap: most workgroups K20a / K20b launch (0: the samples / splits and the CUs
// decide)
static GridCap g_afm_cap;

// K20b's row split, a function of B alone: ceil(B / 32) rows a split
static RowSplit afm_bwd_split(int64_t B) { return row_split(B, kAfmMaxSplits, 1, 1); }

static int64_t afm_stride(int d, int A) { return pad4((int64_t)A * d + A + d); }

template <int NU, int NC>
static int launch_afm_fwd(const float* X, int64_t B, int F, int d, const float* W, const float* h,
                          int A, const float* pv, float* y, float* V, float* ML, int drop,
                          const DropSite& dr, hipStream_t st, const char* what) {
  using L = AfmLds<NU, NC>;
  auto floats = [](int F_, int nsl_) { return L::end_x(F_, nsl_) + 16 * nsl_ + kAfmThreads; };
  const int nsl = afm_slabs(F);
  const size_t lds = (size_t)floats(F, nsl) * sizeof(float);
  const size_t lds_max = (size_t)floats(kAfmMaxF, afm_slabs(kAfmMaxF)) * sizeof(float);
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(afm_fwd_kernel<NU, NC>, kAfmThreads, lds_max, cache, &per_cu, what)) return -1;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((afm_fwd_kernel<NU, NC>), dim3(g_afm_cap.grid(B, most)), dim3(kAfmThreads), lds, st,
                     X, B, F, d, W, h, A, pv, y, V, ML, nsl, drop, dr);
  return launch_status(what);
}

// K20b's waves a workgroup: the most of 16, 8, 4 that the form's registers allow without
// scratch (16 waves leave 128 registers a lane: the forms with NU NC <= 2; 8 waves 256: every
// form but NU = NC = 4) and whose LDS (the waves' dX copies grow with F and d) stays inside
// kAfmLdsBudget. A function of the shape alone, like every sum's order.
constexpr size_t kAfmLdsBudget = 128 * 1024;

template <int NU, int NC>
static size_t afm_bwd_lds(int F, int waves) {
  using L = AfmLds<NU, NC>;
  return ((size_t)L::end_x(F, afm_slabs(F)) + (size_t)waves * std::max(F, L::AP) * L::DP) *
         sizeof(float);
}

template <int NU, int NC, int WV>
static int launch_afm_bwd(const float* X, int64_t B, int F, int d, const float* W, const float* h,
                          int A, const float* pv, const float* V, const float* ML, const float* gy,
                          float* dX, float* partials, int drop, const DropSite& dr, hipStream_t st,
                          const char* what) {
  using L = AfmLds<NU, NC>;
  const int nsl = afm_slabs(F), big = std::max(F, L::AP) * L::DP;
  const size_t lds = afm_bwd_lds<NU, NC>(F, WV);
  const size_t lds_max = std::min(afm_bwd_lds<NU, NC>(kAfmMaxF, WV), kAfmLdsBudget);
  static int cache[kMaxDev] = {};
  if (prepare_launch(afm_bwd_kernel<NU, NC, WV>, 64 * WV, lds_max, cache, nullptr, what)) return -1;
  const RowSplit sp = afm_bwd_split(B);
  hipLaunchKernelGGL((afm_bwd_kernel<NU, NC, WV>), dim3(g_afm_cap.grid(sp.splits, sp.splits)),
                     dim3(64 * WV), lds, st, X, B, F, d, W, h, A, pv, V, ML, gy, dX, partials,
                     afm_stride(d, A), sp.rows, sp.splits, nsl, big, drop, dr);
  return launch_status(what);
}

template <int NU, int NC>
static int launch_afm_bwd_waves(const float* X, int64_t B, int F, int d, const float* W,
                                const float* h, int A, const float* pv, const float* V,
                                const float* ML, const float* gy, float* dX, float* partials,
                                int drop, const DropSite& dr, hipStream_t st, const char* what) {
  if constexpr (NU * NC <= 2) {
    if (afm_bwd_lds<NU, NC>(F, 16) <= kAfmLdsBudget)
      return launch_afm_bwd<NU, NC, 16>(X, B, F, d, W, h, A, pv, V, ML, gy, dX, partials, drop, dr,
                                        st, what);
  }
  if constexpr (NU * NC < 16) {
    if (afm_bwd_lds<NU, NC>(F, 8) <= kAfmLdsBudget)
      return launch_afm_bwd<NU, NC, 8>(X, B, F, d, W, h, A, pv, V, ML, gy, dX, partials, drop, dr,
                                       st, what);
  }
  return launch_afm_bwd<NU, NC, 4>(X, B, F, d, W, h, A, pv, V, ML, gy, dX, partials, drop, dr, st,
                                   what);
}

static int afm_shape_error(const char* what, int32_t F, int32_t d, int32_t A) {
  set_error("%s: shape F %d, d %d, A %d is not in the built set (F 2..%d, d 2..%d, A 1..%d)",
            what, F, d, A, kAfmMaxF, kAfmMaxD, kAfmMaxA);
  return -1;
}

}  // namespace mirec

using namespace mirec;

#define MIREC_AFM_TILES(G, U) G(U, 1) G(U, 2) G(U, 3) G(U, 4)
#define MIREC_AFM_FORMS(G) MIREC_AFM_TILES(G, 1) MIREC_AFM_TILES(G, 2) MIREC_AFM_TILES(G, 3) \
  MIREC_AFM_TILES(G, 4)

extern "C" int32_t mirec_afm_grid_cap(int32_t workgroups) {
  return g_afm_cap.exchange(workgroups);
}

extern "C" int mirec_afm_shape_ok(int32_t F, int32_t d, int32_t A) {
  return F >= 2 && F <= kAfmMaxF && d >= 2 && d <= kAfmMaxD && A >= 1 && A <= kAfmMaxA;
}

extern "C" int32_t mirec_afm_bwd_splits(int64_t B, int32_t F, int32_t d, int32_t A) {
  if (B <= 0 || F < 1 || d < 1 || A < 1) return 0;
  return afm_bwd_split(B).splits;
}

extern "C" int64_t mirec_afm_bwd_stride(int32_t d, int32_t A) {
  if (d < 0 || A < 0) return -1;
  return afm_stride(d, A);
}

extern "C" int mirec_afm_fwd_f32(const float* X, int64_t B, int32_t F, int32_t d, const float* W,
                                 const float* h, int32_t A, const float* pv, float* y, float* V,
                                 float* ML, float p, uint64_t seed, int64_t* counter,
                                 int64_t* drawn, void* stream) {
  const char* what = "mirec_afm_fwd_f32";
  if (!mirec_afm_shape_ok(F, d, A)) return afm_shape_error(what, F, d, A);
  if (B < 0 || !X || !W || !h || !pv || !y || !V || !ML) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  DropSite dr;
  if (drop_site_or_off(p, seed, counter, drawn, &dr, what)) return -1;
  if (B == 0) return 0;
  const int nu = (d + 15) / 16, nc = (A + 15) / 16, drop = p != 0.f;
  hipStream_t st = (hipStream_t)stream;
#define MIREC_AFM(U, C)      \
  if (nu == U && nc == C)    \
    return launch_afm_fwd<U, C>(X, B, F, d, W, h, A, pv, y, V, ML, drop, dr, st, what);
  MIREC_AFM_FORMS(MIREC_AFM)
#undef MIREC_AFM
  return -1;
}

extern "C" int mirec_afm_bwd_f32(const float* X, int64_t B, int32_t F, int32_t d, const float* W,
                                 const float* h, int32_t A, const float* pv, const float* V,
                                 const float* ML, const float* gy, float* dX, float* partials,
                                 float p, uint64_t seed, int64_t* drawn, int64_t* counter,
                                 void* stream) {
  const char* what = "mirec_afm_bwd_f32";
  if (!mirec_afm_shape_ok(F, d, A)) return afm_shape_error(what, F, d, A);
  if (B <= 0 || !X || !W || !h || !pv || !V || !ML || !gy || !dX || !partials) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  DropSite dr;
  if (drop_site_or_off(p, seed, counter, drawn, &dr, what)) return -1;
  const int nu = (d + 15) / 16, nc = (A + 15) / 16, drop = p != 0.f;
  hipStream_t st = (hipStream_t)stream;
#define MIREC_AFM(U, C)      \
  if (nu == U && nc == C)    \
    return launch_afm_bwd_waves<U, C>(X, B, F, d, W, h, A, pv, V, ML, gy, dX, partials, drop, dr, \
                                      st, what);
  MIREC_AFM_FORMS(MIREC_AFM)
#undef MIREC_AFM
  return -1;
}
