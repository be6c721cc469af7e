// K19 — DCN's cross network and the cross slice of its prediction head (reference
// dcn.py:78-99, 101-113). With x_0 [B, n], w_l and b_l [n] for l < L:
//   s_l = x_l . w_l,   x_{l+1} = x_0 s_l + b_l + x_l,   y = x_L . wp
// The reference runs ~5 small torch ops a layer and autograd keeps every x_l [B, n]. Here a
// wave owns a row: lane j holds elements j, j + 64, ... of x_0 in registers (4-byte loads, so
// no alignment is asked of a row), and one launch does each pass.
//
// Every x_l is an affine image of x_0: x_l = c_l x_0 + beta_l with c_0 = 1, c_{l+1} = c_l + s_l
// (per row) and beta_l = sum_{k<l} b_k (the same for every row). So
//   s_l = c_l (x_0 . w_l) + beta_l . w_l         y = c_L (x_0 . wp) + beta_L . wp
// and a row needs the L + 1 dot products of x_0 with fixed vectors (independent of one
// another: one pass over the registers, then L + 1 interleaved DPP wave sums) and a scalar
// recurrence. The batch-wide scalars q_l = beta_l . w_l are summed by every workgroup in its
// prologue, in an order fixed by n alone.
//
//   K19a cross_fwd_kernel   256 threads, a row per wave, workgroups stride over groups of 4
//                           rows. W, wp (zero-padded to 64 NK) and beta_L sit in LDS. Writes
//                           S [B, L], y (head mode) and x_L = c_L x_0 + beta_L (plain mode).
//   K19b cross_bwd_kernel   a workgroup of WV waves (8 up to n = 256, 4 above) per split of the
//                           rows, wave w taking rows r0 + w, r0 + w + WV, ... With g_L = gy wp + gL, h = g_L . x_0 =
//                           gy (x_0 . wp) + gL . x_0 and p_l = x_0 . w_l:
//                             t_l = g_{l+1} . x_0 = h + sum_{k>l} t_k p_k      (l = L-1 .. 0)
//                             dx0 = c_L g_L + sum_l (t_l c_l) w_l
//                           (the recurrence g_l = g_{l+1} + t_l w_l, dx0 = g_0 + sum_l s_l
//                           g_{l+1}, with the sums exchanged). The batch sums collapse to
//                             dW_l  = sum_rows (t_l c_l) x_0 + beta_l sum_rows t_l
//                             dB_l  = sum_rows gL + wp sum_rows gy + sum_{k>l} w_k sum_rows t_k
//                             dwp   = sum_rows (gy c_L) x_0 + beta_L sum_rows gy
//                           so a wave keeps L + 2 register accumulators of its NK elements
//                           (x_0^T times a per-row scalar, and sum gL) and L + 1 scalars. The
//                           workgroup's waves are added through LDS in wave order, the
//                           constant terms go on, and split s's [dW | dB | dwp] is stored;
//                           mirec_linear_grad_finish_f32 adds the splits in order.
//
// Saved between the passes: S only. No [B, n] tensor per layer exists in either pass. Every
// sum has an order fixed by (B, n, L): the lane's elements in order, the DPP tree, a
// wave's rows in order, the waves in order, the splits in order. No float atomics.
//
// The loops over a row are layer-outer with every load unconditional (a clamped index, the
// value masked afterwards): one uniform branch a layer and NK independent LDS reads or global
// loads behind it. Guarding each element's load with its own branch serialises the loads.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch in any
// form): dynamic LDS, K19a (L + 2) 64 NK floats + 45 (<= 41140 B), K19b (L + 1 + WV) 64 NK
// floats + 9 (WV + 1) (<= 53428 B at NK = 16, WV = 4). VGPRs: K19a 36 - 110; K19b 111 / 129 /
// 186 at NK = 1 / 2 / 4 (eight waves), 256 + 58 / 131 / 232 AGPRs at NK = 8 / 12 / 16 (four
// waves: the 8 NK accumulators and 4 NK row registers do not fit 256 registers a lane).
#include "common.h"
#include "rowsplit.h"

#include <algorithm>

namespace mirec {

constexpr int kCrossLMax = 8;
constexpr int kCrossQ = kCrossLMax + 1;        // scalars a row or a split carries
constexpr int kCrossFwdThreads = 256;
constexpr int kCrossFwdWaves = kCrossFwdThreads / 64;
constexpr int kCrossBwdWaves = 8;         // K19b's waves up to NK = 4; wider rows take 4
constexpr int kCrossBwdWideWaves = 4;     // (512 registers a lane for the accumulators)
constexpr int kCrossMaxSplits = 32;

// The sum of one float per lane over the wave, the same value in every lane: two quad
// permutes and two row rotations leave each 16-lane row's total in all its lanes, two row
// broadcasts carry the totals up to lane 63, one readlane hands it to everyone. Six DPP adds
// on the VALU: the L + 2 dots of a row cost no LDS round trip (a __shfl_xor is a ds_bpermute).
__device__ __forceinline__ float cross_wave_sum(float x) {
#define MIREC_DPP_ADD(ctrl, rows)                                                             \
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, rows, 0xf, false))
  MIREC_DPP_ADD(0xb1, 0xf);     // quad_perm:[1,0,3,2]
  MIREC_DPP_ADD(0x4e, 0xf);     // quad_perm:[2,3,0,1]
  MIREC_DPP_ADD(0x124, 0xf);    // row_ror:4
  MIREC_DPP_ADD(0x128, 0xf);    // row_ror:8
  MIREC_DPP_ADD(0x142, 0xa);    // row_bcast:15 into rows 1 and 3
  MIREC_DPP_ADD(0x143, 0xc);    // row_bcast:31 into rows 2 and 3
#undef MIREC_DPP_ADD
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63));
}

// ---------------------------------------------------------------- K19a
template <int NK>
__global__ __launch_bounds__(kCrossFwdThreads) void cross_fwd_kernel(
    const float* __restrict__ x0, int64_t B, int n, const float* __restrict__ W,
    const float* __restrict__ Bv, int L, const float* __restrict__ wp, float* __restrict__ S,
    float* __restrict__ y, float* __restrict__ xL, int64_t groups) {
  constexpr int NP = 64 * NK;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW = smem;                  // [L][NP]
  float* sP = sW + L * NP;           // wp [NP]
  float* sBeta = sP + NP;            // beta_L [NP]
  float* sRed = sBeta + NP;          // [waves][kCrossQ]
  float* sQ = sRed + kCrossFwdWaves * kCrossQ;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  // stage the weights; q_l = beta_l . w_l (l < L) and q_8 = beta_L . wp
  float part[kCrossQ];
#pragma unroll
  for (int q = 0; q < kCrossQ; ++q) part[q] = 0.f;
  for (int i = tid; i < NP; i += kCrossFwdThreads) {
    const bool in = i < n;
    const int ic = in ? i : n - 1;       // every load unconditional (in flight together)
    float beta = 0.f;
#pragma unroll
    for (int l = 0; l < kCrossLMax; ++l)
      if (l < L) {
        const float wl = W[l * n + ic], bl = Bv[l * n + ic];
        const float wv = in ? wl : 0.f;
        sW[l * NP + i] = wv;
        part[l] += beta * wv;
        beta += in ? bl : 0.f;
      }
    float pv = 0.f;
    if (wp) pv = wp[ic];
    pv = in ? pv : 0.f;
    sP[i] = pv;
    part[kCrossLMax] += beta * pv;
    sBeta[i] = beta;
  }
#pragma unroll
  for (int q = 0; q < kCrossQ; ++q) part[q] = cross_wave_sum(part[q]);
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < kCrossQ; ++q) sRed[w * kCrossQ + q] = part[q];
  }
  __syncthreads();
  if (tid < kCrossQ) {
    float a = 0.f;
    for (int v = 0; v < kCrossFwdWaves; ++v) a += sRed[v * kCrossQ + tid];
    sQ[tid] = a;
  }
  __syncthreads();
  float q[kCrossQ];
#pragma unroll
  for (int i = 0; i < kCrossQ; ++i) q[i] = sQ[i];

  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t b = g * kCrossFwdWaves + w;
    if (b >= B) continue;
    const float* xr = x0 + b * n;
    float x[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) {       // clamped, unconditional loads: all in flight at once
      const int i = lane + 64 * k;
      const float v = xr[i < n ? i : n - 1];
      x[k] = i < n ? v : 0.f;
    }
    float p[kCrossQ];
#pragma unroll
    for (int i = 0; i < kCrossQ; ++i) p[i] = 0.f;
    // one uniform branch a layer, its NK LDS reads and multiply-adds in one block
#pragma unroll
    for (int l = 0; l < kCrossLMax; ++l)
      if (l < L) {
#pragma unroll
        for (int k = 0; k < NK; ++k) p[l] += x[k] * sW[l * NP + lane + 64 * k];
      }
    if (wp) {
#pragma unroll
      for (int k = 0; k < NK; ++k) p[kCrossLMax] += x[k] * sP[lane + 64 * k];
    }
#pragma unroll
    for (int l = 0; l < kCrossLMax; ++l)
      if (l < L) p[l] = cross_wave_sum(p[l]);
    if (wp) p[kCrossLMax] = cross_wave_sum(p[kCrossLMax]);
    float c = 1.f;
#pragma unroll
    for (int l = 0; l < kCrossLMax; ++l)
      if (l < L) {
        const float s = c * p[l] + q[l];
        if (lane == 0) S[b * L + l] = s;
        c += s;
      }
    if (wp && lane == 0) y[b] = c * p[kCrossLMax] + q[kCrossLMax];
    if (xL) {
      float* xo = xL + b * n;
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int i = lane + 64 * k;
        if (i < n) xo[i] = c * x[k] + sBeta[i];
      }
    }
  }
}

// ---------------------------------------------------------------- K19b
template <int NK, int WV>
__global__ __launch_bounds__(64 * WV) void cross_bwd_kernel(
    const float* __restrict__ x0, int64_t B, int n, const float* __restrict__ W,
    const float* __restrict__ Bv, int L, const float* __restrict__ S,
    const float* __restrict__ wp, const float* __restrict__ gy, const float* __restrict__ gL,
    float* __restrict__ dx0, float* __restrict__ partials, int64_t stride, int64_t rows,
    int splits) {
  constexpr int NP = 64 * NK, TH = 64 * WV;
  constexpr int NE = (NP + TH - 1) / TH;   // elements a thread ends
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* sW = smem;                          // [L][NP]
  float* sP = sW + L * NP;                   // wp [NP]
  float* sRedV = sP + NP;                    // [waves][NP]
  float* sRedS = sRedV + WV * NP;   // [waves][kCrossQ]
  float* sT = sRedS + WV * kCrossQ;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool head = wp != nullptr;

  for (int i = tid; i < NP; i += TH) {
    const bool in = i < n;
    const int ic = in ? i : n - 1;
    for (int l = 0; l < L; ++l) {
      const float wl = W[l * n + ic];
      sW[l * NP + i] = in ? wl : 0.f;
    }
    float pv = 0.f;
    if (head) pv = wp[ic];
    sP[i] = in ? pv : 0.f;
  }
  __syncthreads();

  // the waves' partial vectors added in wave order: thread tid ends elements tid + TH e
  auto reduce = [&](const float (&v)[NK], float (&out)[NE]) {
#pragma unroll
    for (int k = 0; k < NK; ++k) sRedV[w * NP + lane + 64 * k] = v[k];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + TH * e;
      float a = 0.f;
      if (i < NP)
        for (int v8 = 0; v8 < WV; ++v8) a += sRedV[v8 * NP + i];
      out[e] = a;
    }
    __syncthreads();
  };

  for (int s = blockIdx.x; s < splits; s += gridDim.x) {
    const int64_t r0 = (int64_t)s * rows, r1 = r0 + rows < B ? r0 + rows : B;
    float A[kCrossLMax][NK], Ap[NK], G[NK], T[kCrossQ];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l) A[l][k] = 0.f;
      Ap[k] = 0.f;
      G[k] = 0.f;
    }
#pragma unroll
    for (int i = 0; i < kCrossQ; ++i) T[i] = 0.f;      // T[l] = sum t_l, T[8] = sum gy

    for (int64_t b = r0 + w; b < r1; b += WV) {
      const float* xr = x0 + b * n;
      const float* gr = gL ? gL + b * n : nullptr;
      float x[NK], gl[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) {     // clamped, unconditional loads: all in flight at once
        const int i = lane + 64 * k;
        const float v = xr[i < n ? i : n - 1];
        x[k] = i < n ? v : 0.f;
        gl[k] = 0.f;
      }
      if (gr) {
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          const int i = lane + 64 * k;
          const float v = gr[i < n ? i : n - 1];
          gl[k] = i < n ? v : 0.f;
        }
      }
      const float gyb = head ? gy[b] : 0.f;
      float sl[kCrossLMax];
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l) sl[l] = l < L ? S[b * L + l] : 0.f;
      float p[kCrossLMax], pp = 0.f, a = 0.f;
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l) p[l] = 0.f;
      // one uniform branch a layer, its NK LDS reads and multiply-adds in one block
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l)
        if (l < L) {
#pragma unroll
          for (int k = 0; k < NK; ++k) p[l] += x[k] * sW[l * NP + lane + 64 * k];
        }
      if (head) {
#pragma unroll
        for (int k = 0; k < NK; ++k) pp += x[k] * sP[lane + 64 * k];
      }
      if (gr) {
#pragma unroll
        for (int k = 0; k < NK; ++k) a += x[k] * gl[k];
      }
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l)
        if (l < L) p[l] = cross_wave_sum(p[l]);
      if (head) pp = cross_wave_sum(pp);
      if (gr) a = cross_wave_sum(a);
      // c_l, t_l and the coefficients u_l = t_l c_l
      float c[kCrossLMax + 1], u[kCrossLMax];
      c[0] = 1.f;
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l) c[l + 1] = c[l] + sl[l];   // sl = 0 past L
      const float h = gyb * pp + a;
      float acc = h;
#pragma unroll
      for (int l = kCrossLMax - 1; l >= 0; --l) {
        u[l] = 0.f;
        if (l < L) {
          const float t = acc;
          acc += t * p[l];
          u[l] = t * c[l];
          T[l] += t;
        }
      }
      const float cL = c[kCrossLMax], up = gyb * cL;
      T[kCrossLMax] += gyb;
      float* dr = dx0 + b * n;
      float d[NK];
#pragma unroll
      for (int k = 0; k < NK; ++k) d[k] = cL * (gl[k] + gyb * sP[lane + 64 * k]);
#pragma unroll
      for (int l = 0; l < kCrossLMax; ++l)
        if (l < L) {
#pragma unroll
          for (int k = 0; k < NK; ++k) {
            d[k] += u[l] * sW[l * NP + lane + 64 * k];
            A[l][k] += u[l] * x[k];
          }
        }
#pragma unroll
      for (int k = 0; k < NK; ++k) {
        const int i = lane + 64 * k;
        Ap[k] += up * x[k];
        G[k] += gl[k];
        if (i < n) dr[i] = d[k];
      }
    }

    // the split's sums: scalars first, then one vector at a time through sRedV
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kCrossQ; ++i) sRedS[w * kCrossQ + i] = T[i];
    }
    __syncthreads();
    if (tid < kCrossQ) {
      float a = 0.f;
      for (int v8 = 0; v8 < WV; ++v8) a += sRedS[v8 * kCrossQ + tid];
      sT[tid] = a;
    }
    __syncthreads();
    float* P = partials + (int64_t)s * stride;
    const int Ln = L * n;
    float Gs[NE], o[NE], beta[NE];
    reduce(G, Gs);
#pragma unroll
    for (int e = 0; e < NE; ++e) beta[e] = 0.f;
#pragma unroll
    for (int l = 0; l < kCrossLMax; ++l)
      if (l < L) {
        reduce(A[l], o);
#pragma unroll
        for (int e = 0; e < NE; ++e) {
          const int i = tid + TH * e;
          if (i < n) {
            P[l * n + i] = o[e] + beta[e] * sT[l];
            beta[e] += Bv[l * n + i];
          }
        }
      }
    if (head) reduce(Ap, o);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const int i = tid + TH * e;
      if (i < n) {
        P[2 * Ln + i] = head ? o[e] + beta[e] * sT[kCrossLMax] : 0.f;
        float run = Gs[e] + sT[kCrossLMax] * sP[i];
        for (int l = L - 1; l >= 0; --l) {
          P[Ln + l * n + i] = run;
          run += sT[l] * sW[l * NP + i];
        }
      }
    }
    for (int64_t i = 2 * Ln + n + tid; i < stride; i += TH) P[i] = 0.f;
    __syncthreads();                         // sT and sRedS are reused by the next split
  }
}

// ---------------------------------------------------------------- host side
// mirec_cross_grid_cap: most workgroups K19a / K19b launch (0: the rows / splits and the CUs
// decide)
static GridCap g_cross_cap;

// the built register tiles of n: 64 NK >= n
static int cross_nk(int n) {
  const int t = (n + 63) / 64;
  return t <= 1 ? 1 : t <= 2 ? 2 : t <= 4 ? 4 : t <= 8 ? 8 : t <= 12 ? 12 : 16;
}

// K19b's row split, a function of B alone: at most kCrossMaxSplits splits, each a multiple of
// eight rows
static RowSplit cross_bwd_split(int64_t B) {
  return row_split(B, kCrossMaxSplits, kCrossBwdWaves, kCrossBwdWaves);
}

template <int NK>
static int launch_cross_fwd(const float* x0, int64_t B, int n, const float* W, const float* Bv,
                            int L, const float* wp, float* S, float* y, float* xL,
                            hipStream_t st, const char* what) {
  const size_t lds =
      ((size_t)(L + 2) * 64 * NK + (kCrossFwdWaves + 1) * kCrossQ) * sizeof(float);
  constexpr size_t lds_max =
      ((size_t)(kCrossLMax + 2) * 64 * NK + (kCrossFwdWaves + 1) * kCrossQ) * sizeof(float);
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(cross_fwd_kernel<NK>, kCrossFwdThreads, lds_max, cache, &per_cu, what))
    return -1;
  const int64_t groups = (B + kCrossFwdWaves - 1) / kCrossFwdWaves;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((cross_fwd_kernel<NK>), dim3(g_cross_cap.grid(groups, most)),
                     dim3(kCrossFwdThreads), lds, st, x0, B, n, W, Bv, L, wp, S, y, xL, groups);
  return launch_status(what);
}

template <int NK, int WV>
static int launch_cross_bwd(const float* x0, int64_t B, int n, const float* W, const float* Bv,
                            int L, const float* S, const float* wp, const float* gy,
                            const float* gL, float* dx0, float* partials, hipStream_t st,
                            const char* what) {
  const size_t lds =
      ((size_t)(L + 1 + WV) * 64 * NK + (WV + 1) * kCrossQ) * sizeof(float);
  constexpr size_t lds_max =
      ((size_t)(kCrossLMax + 1 + WV) * 64 * NK + (WV + 1) * kCrossQ) * sizeof(float);
  static int cache[kMaxDev] = {};
  if (prepare_launch(cross_bwd_kernel<NK, WV>, 64 * WV, lds_max, cache, nullptr, what))
    return -1;
  const RowSplit sp = cross_bwd_split(B);
  hipLaunchKernelGGL((cross_bwd_kernel<NK, WV>), dim3(g_cross_cap.grid(sp.splits, sp.splits)),
                     dim3(64 * WV), lds, st, x0, B, n, W, Bv, L, S, wp, gy, gL, dx0,
                     partials, mirec_cross_bwd_stride(n, L), sp.rows, sp.splits);
  return launch_status(what);
}

static int cross_shape_error(const char* what, int32_t n, int32_t L) {
  set_error("%s: shape n %d, L %d is not in the built set (n 2..1024, L 1..%d)", what, n, L,
            kCrossLMax);
  return -1;
}

}  // namespace mirec

using namespace mirec;

#define MIREC_CROSS_FORMS(F) F(1) F(2) F(4) F(8) F(12) F(16)

extern "C" int32_t mirec_cross_grid_cap(int32_t workgroups) {
  return g_cross_cap.exchange(workgroups);
}

extern "C" int mirec_cross_shape_ok(int32_t n, int32_t L) {
  return n >= 2 && n <= 1024 && L >= 1 && L <= kCrossLMax;
}

extern "C" int mirec_cross_fwd_f32(const float* x0, int64_t B, int32_t n, const float* W,
                                   const float* Bv, int32_t L, const float* wp, float* S,
                                   float* y, float* xL, void* stream) {
  const char* what = "mirec_cross_fwd_f32";
  if (!mirec_cross_shape_ok(n, L)) return cross_shape_error(what, n, L);
  if (B < 0 || !x0 || !W || !Bv || !S || (wp && !y) || (!wp && !xL)) {
    set_error("%s: bad arguments (S always; y with wp; xL when wp is NULL)", what);
    return -1;
  }
  if (B == 0) return 0;
  const int nk = cross_nk(n);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CROSS(K) \
  if (nk == K) return launch_cross_fwd<K>(x0, B, n, W, Bv, L, wp, S, y, xL, st, what);
  MIREC_CROSS_FORMS(MIREC_CROSS)
#undef MIREC_CROSS
  return -1;
}

extern "C" int32_t mirec_cross_bwd_splits(int64_t B, int32_t n, int32_t L) {
  if (B <= 0 || n < 1 || L < 1) return 0;
  return cross_bwd_split(B).splits;
}

extern "C" int64_t mirec_cross_bwd_stride(int32_t n, int32_t L) {
  if (n < 0 || L < 0) return -1;
  return pad4((int64_t)(2 * L + 1) * n);
}

extern "C" int mirec_cross_bwd_f32(const float* x0, int64_t B, int32_t n, const float* W,
                                   const float* Bv, int32_t L, const float* S, const float* wp,
                                   const float* gy, const float* gL, float* dx0, float* partials,
                                   void* stream) {
  const char* what = "mirec_cross_bwd_f32";
  if (!mirec_cross_shape_ok(n, L)) return cross_shape_error(what, n, L);
  if (B <= 0 || !x0 || !W || !Bv || !S || !dx0 || !partials || (wp != nullptr) != (gy != nullptr) ||
      (!gy && !gL)) {
    set_error("%s: bad arguments (wp and gy together; at least one of gy, gL)", what);
    return -1;
  }
  const int nk = cross_nk(n);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_CROSS(K)                                                                         \
  if (nk == K)                                                                                 \
    return launch_cross_bwd<K, (K <= 4 ? kCrossBwdWaves : kCrossBwdWideWaves)>(                \
        x0, B, n, W, Bv, L, S, wp, gy, gL, dx0, partials, st, what);
  MIREC_CROSS_FORMS(MIREC_CROSS)
#undef MIREC_CROSS
  return -1;
}
