// K16 — NGCF's bi-interaction layer (reference ngcf.py:132-147 and BiGNNLayer,
// layers.py:174-197) on fp32 MFMA. With x = A_hat E_l already formed by K7 (graph.hip),
// one layer is
//   z       = (E_l + x) W1^T + b1 + (x * E_l) W2^T + b2
//   m       = dropout(LeakyReLU_0.2(z))
//   E_{l+1} = m / max(||m||_2, 1e-12)                          per row
// which the reference runs as about ten passes over [N, d] tensors. Three kernels, all in
// K11's shape (linear.hip: the weight in LDS as Bs[n][k] with row stride K + 4, eight waves
// walking 16-row slabs on their own, v_mfma_f32_16x16x4_f32):
//
//   K16a ngcf_fwd_kernel    B = [W1 | W2] as one [d_out, 2 d_in] operand; the A rows
//                           (E_l + x | x * E_l) are formed in registers while loading;
//                           bias, LeakyReLU, dropout draw, row norm and scale in the
//                           epilogue. Writes E_{l+1} into its column slice of the [N, D]
//                           concat buffer (row stride D), optionally a contiguous copy for
//                           the next K7, and ||m|| to [N].
//   K16b ngcf_bwd_kernel    per row g_z from (G, E_{l+1}, ||m||) and the redrawn keep bits
//                           (sign(E_{l+1}) = sign(z) wherever kept, so z is not stored);
//                           stores g_z; g_a | g_p = g_z [W1 | W2] (the weights transposed
//                           into LDS); writes dE_direct = g_a + g_p * x (+ add) and
//                           g_x = g_a + g_p * E_l. One K7 launch then gives
//                           dE_l = A_hat'^T g_x + dE_direct.
//   K16c ngcf_wgrad_kernel  split-K over the node rows: workgroup b owns rows
//                           [b R, (b + 1) R) and stores its [d_out, 2 d_in] partial of
//                           g_z^T (E_l + x | x * E_l); mirec_linear_grad_finish_f32 adds the
//                           partials in block order and forms the bias column sum.
//
// Every sum has a fixed order that depends only on the shapes: the MFMA k order, the
// row norm as an xor butterfly over the row's 16 lanes (both partners add the same two
// values, so all lanes hold the same bits) after the column tiles in tile order, the
// K16c rows in row order. No float atomics.
//
// Message dropout: the shared counter-based draw (drop.h), element e = row * d_out + column.
//
// Rows operands are (lo, hi, split, ld): row r at lo + r ld below split, else at
// hi + (r - split) ld — the two embedding tables as E_0, a column slice of the concat
// buffer (ld = D) or of the two output gradients.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; LDS is dynamic,
// (rows of Bs) x (K + 4) floats). No kernel uses scratch:
//   (d_in, d_out)   K16a VGPR p=0 / p>0, LDS      K16b VGPR p=0 / p>0, LDS      K16c VGPR
//   ( 64,  64)      148 / 154,  33792 B            122 / 116,  34816 B            59
//   ( 64, 128)      168 / 176,  67584 B            138 / 136,  67584 B            85
//   (128,  64)      144 / 150,  66560 B            150 / 152,  69632 B            74
//   (128, 128)      178 / 252, 133120 B            168 / 168, 135168 B           122
// (K16c uses no LDS; eight waves a workgroup leave each wave 256 registers.)
#include "common.h"
#include "drop.h"
#include "mfma.h"
#include "rowsplit.h"

#include <algorithm>

namespace mirec {

constexpr int kNgThreads = 512;           // eight waves
constexpr int kNgWaves = kNgThreads / 64;

struct RowsLd {
  float* lo;
  float* hi;
  int64_t split;
  int64_t ld;
  __device__ __forceinline__ float* row(int64_t r) const {
    return r < split ? lo + r * ld : hi + (r - split) * ld;
  }
};

// ---------------------------------------------------------------- K16a
template <int DI, int DO, bool DROP>
__global__ __launch_bounds__(kNgThreads) void ngcf_fwd_kernel(
    const RowsLd E, const float* __restrict__ X, int64_t M, const float* __restrict__ W1,
    const float* __restrict__ b1, const float* __restrict__ W2, const float* __restrict__ b2,
    const RowsLd out, float* __restrict__ copy, float* __restrict__ nrm, const DropSite dr) {
  constexpr int K = 2 * DI, KP = K + 4, NU = K / 16, NH = DI / 16, NC = DO / 16;
  extern __shared__ __attribute__((aligned(16))) float Bs[];   // [DO][KP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t slabs = (M + 15) / 16;
  const int64_t nw = (int64_t)gridDim.x * kNgWaves;
  int64_t s = (int64_t)blockIdx.x * kNgWaves + w;
  // lane (li, lk): row 16 s + li, floats 16u + 4lk .. +3 of (E + x) for u < NH, of x * E after
  auto load_a = [&](float4 (&a)[NU], int64_t ss) {
    const int64_t r = 16 * ss + li;
    const bool ok = ss < slabs && r < M;
    const float* e = E.row(ok ? r : 0) + 4 * lk;
    const float* x = X + (ok ? r : 0) * DI + 4 * lk;
#pragma unroll
    for (int u = 0; u < NH; ++u) {
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 ev = ok ? *reinterpret_cast<const float4*>(e + 16 * u) : z4;
      const float4 xv = ok ? *reinterpret_cast<const float4*>(x + 16 * u) : z4;
      a[u] = make_float4(ev.x + xv.x, ev.y + xv.y, ev.z + xv.z, ev.w + xv.w);
      a[NH + u] = make_float4(xv.x * ev.x, xv.y * ev.y, xv.z * ev.z, xv.w * ev.w);
    }
  };
  float4 a[NU];
  load_a(a, s);                           // in flight with the staging

  for (int e = tid; e < DO * K / 4; e += kNgThreads) {
    const int n = e / (K / 4), k4 = (e % (K / 4)) * 4;
    const float* src = k4 < DI ? W1 + (int64_t)n * DI + k4 : W2 + (int64_t)n * DI + (k4 - DI);
    *reinterpret_cast<float4*>(&Bs[n * KP + k4]) = *reinterpret_cast<const float4*>(src);
  }
  float bv[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) bv[c] = b1[16 * c + li] + b2[16 * c + li];
  uint64_t key = 0;
  if (DROP) {
    const int64_t cv = dr.counter[0];
    if (blockIdx.x == 0 && tid == 0) dr.drawn[0] = cv;
    key = drop_key(dr.seed, cv);
  }
  __syncthreads();

  for (; s < slabs; s += nw) {
    constexpr bool kPre = NU <= 8;        // d_in = 128: no room for a second A slab
    float4 an[NU];                        // the next slab's A rows (kPre only; unused otherwise)
    if constexpr (kPre) load_a(an, s + nw);
    floatx4 acc[NC];
    mfma_slab<NU, NC, KP>(a, Bs, li, lk, acc);
    // C layout: acc[c][i] = z[16 s + 4lk + i][16c + li] (before the bias)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = 16 * s + 4 * lk + i;
      float m[NC];
      float ss = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const float z = acc[c][i] + bv[c];
        float h = z > 0.f ? z : 0.2f * z;
        if (DROP)
          h = drop_keep(key, (uint64_t)r * DO + 16 * c + li, dr.thr) ? h * dr.scale : 0.f;
        m[c] = h;
        ss = fmaf(h, h, ss);
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) ss += __shfl_xor(ss, off, 64);
      const float n = sqrtf(ss);
      const float den = fmaxf(n, 1e-12f);
      if (r < M) {
        float* o = out.row(r) + li;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const float y = m[c] / den;
          o[16 * c] = y;
          if (copy) copy[r * DO + 16 * c + li] = y;
        }
        if (li == 0) nrm[r] = n;
      }
    }
    if constexpr (kPre) {
#pragma unroll
      for (int u = 0; u < NU; ++u) a[u] = an[u];
    } else {
      if (s + nw < slabs) load_a(a, s + nw);
    }
  }
}

// ---------------------------------------------------------------- K16b
template <int DI, int DO, bool DROP>
__global__ __launch_bounds__(kNgThreads) void ngcf_bwd_kernel(
    const RowsLd G, const RowsLd En, const float* __restrict__ nrm, int64_t M,
    const float* __restrict__ W1, const float* __restrict__ W2, const RowsLd El,
    const float* __restrict__ X, const RowsLd add, float* __restrict__ gz,
    float* __restrict__ dE, float* __restrict__ gx, const DropSite dr) {
  constexpr int KP = DO + 4, NU = DO / 16, NC = 2 * DI / 16, NH = DI / 16;
  extern __shared__ __attribute__((aligned(16))) float Bs[];   // [2 DI][KP]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t slabs = (M + 15) / 16;
  const int64_t nw = (int64_t)gridDim.x * kNgWaves;

  // Bs[n][k] = W1[k][n] for n < DI, W2[k][n - DI] after (W row-major [DO][DI])
  for (int e = tid; e < 2 * DO * DI / 4; e += kNgThreads) {
    const int h = e / (DO * DI / 4), q = e % (DO * DI / 4);
    const int k = q / (DI / 4), n4 = (q % (DI / 4)) * 4;
    const float4 v = *reinterpret_cast<const float4*>((h ? W2 : W1) + (int64_t)k * DI + n4);
    float* b = &Bs[(h * DI + n4) * KP + k];
    b[0] = v.x;
    b[KP] = v.y;
    b[2 * KP] = v.z;
    b[3 * KP] = v.w;
  }
  uint64_t key = 0;
  if (DROP) {
    const int64_t cv = dr.drawn[0];
    if (blockIdx.x == 0 && tid == 0) dr.counter[0] = cv + 1;
    key = drop_key(dr.seed, cv);
  }
  __syncthreads();

  for (int64_t s = (int64_t)blockIdx.x * kNgWaves + w; s < slabs; s += nw) {
    // A rows = g_z in the MFMA's A layout: lane (li, lk) holds row 16 s + li, floats
    // 16u + 4lk .. +3; the row's <E_{l+1}, G> over its four lanes (lk) and their k slices
    float4 a[NU];
    {
      const int64_t r = 16 * s + li;
      const bool ok = r < M;
      const float* g = G.row(ok ? r : 0) + 4 * lk;
      const float* e = En.row(ok ? r : 0) + 4 * lk;
      const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 gv[NU], ev[NU];
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        gv[u] = ok ? *reinterpret_cast<const float4*>(g + 16 * u) : z4;
        ev[u] = ok ? *reinterpret_cast<const float4*>(e + 16 * u) : z4;
      }
      const float nr = ok ? nrm[r] : 1.f;
      float sd = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        sd = fmaf(ev[u].x, gv[u].x, sd);
        sd = fmaf(ev[u].y, gv[u].y, sd);
        sd = fmaf(ev[u].z, gv[u].z, sd);
        sd = fmaf(ev[u].w, gv[u].w, sd);
      }
      sd += __shfl_xor(sd, 16, 64);
      sd += __shfl_xor(sd, 32, 64);
      // d(m / max(||m||, eps)): below the clamp the denominator is the constant eps
      const bool big = nr >= 1e-12f;
      const float den = big ? nr : 1e-12f;
      if (!big) sd = 0.f;
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        bool kp[4] = {true, true, true, true};
        if (DROP) drop_keep4(key, (uint64_t)r * DO + 16 * u + 4 * lk, dr.thr, kp);
        const float sc = DROP ? dr.scale : 1.f;
        auto one = [&](float gq, float eq, bool kq) {
          const float gm = (gq - eq * sd) / den;
          return kq ? gm * sc * (eq > 0.f ? 1.f : 0.2f) : 0.f;
        };
        a[u] = make_float4(one(gv[u].x, ev[u].x, kp[0]), one(gv[u].y, ev[u].y, kp[1]),
                           one(gv[u].z, ev[u].z, kp[2]), one(gv[u].w, ev[u].w, kp[3]));
        if (ok) *reinterpret_cast<float4*>(gz + r * DO + 16 * u + 4 * lk) = a[u];
      }
    }
    floatx4 acc[NC];
    mfma_slab<NU, NC, KP>(a, Bs, li, lk, acc);
    // C layout: acc[c][i] = g_a[16 s + 4lk + i][16c + li] for c < NH, g_p for c - NH
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t r = 16 * s + 4 * lk + i;
      if (r < M) {
        const float* el = El.row(r) + li;
        const float* ad = add.lo ? add.row(r) + li : nullptr;
#pragma unroll
        for (int c = 0; c < NH; ++c) {
          const int64_t o = r * DI + 16 * c + li;
          const float ga = acc[c][i], gp = acc[NH + c][i];
          float d = fmaf(gp, X[o], ga);
          if (ad) d += ad[16 * c];
          dE[o] = d;
          gx[o] = fmaf(gp, el[16 * c], ga);
        }
      }
    }
  }
}

// ---------------------------------------------------------------- K16c
// P[b][n][k] = sum over the rows r of block b, in row order, of g_z[r][n] ap[r][k],
// ap = (E_l + x | x * E_l). Wave w owns the k tiles w JW .. w JW + JW - 1 (JW = 2 DI / 128)
// and every n tile: per four rows, lane (li, lk) supplies g_z[r0 + lk][16 nt + li] as A and
// ap[r0 + lk][16 jt + li] as B; sixteen rows' loads are issued together.
template <int DI, int DO>
__global__ __launch_bounds__(kNgThreads) void ngcf_wgrad_kernel(
    const float* __restrict__ gz, const RowsLd El, const float* __restrict__ X, int64_t M,
    int64_t rows_per_block, float* __restrict__ P) {
  constexpr int K2 = 2 * DI, NN = DO / 16, JW = K2 / 16 / kNgWaves;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int64_t r_beg = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r_end = std::min<int64_t>(M, r_beg + rows_per_block);
  floatx4 acc[NN][JW];
#pragma unroll
  for (int n = 0; n < NN; ++n)
#pragma unroll
    for (int j = 0; j < JW; ++j) acc[n][j] = floatx4{0.f, 0.f, 0.f, 0.f};
  for (int64_t r0 = r_beg; r0 < r_end; r0 += 16) {
    float av[4][NN], bv[4][JW];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int64_t r = r0 + 4 * q + lk;
      const bool ok = r < r_end;
      const float* g = gz + (ok ? r : r_beg) * DO + li;
      const float* e = El.row(ok ? r : r_beg);
      const float* x = X + (ok ? r : r_beg) * DI;
#pragma unroll
      for (int n = 0; n < NN; ++n) av[q][n] = ok ? g[16 * n] : 0.f;
#pragma unroll
      for (int j = 0; j < JW; ++j) {
        const int col = 16 * (w * JW + j) + li;          // of [a | p]
        const int cc = col < DI ? col : col - DI;
        const float ev = e[cc], xv = x[cc];
        bv[q][j] = ok ? (col < DI ? ev + xv : xv * ev) : 0.f;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int n = 0; n < NN; ++n)
#pragma unroll
        for (int j = 0; j < JW; ++j) acc[n][j] = mfma_16x16x4(av[q][n], bv[q][j], acc[n][j]);
  }
  // C layout: acc[n][j][i] = P[16n + 4lk + i][16 (w JW + j) + li]
  float* Pb = P + (int64_t)blockIdx.x * DO * K2;
#pragma unroll
  for (int n = 0; n < NN; ++n)
#pragma unroll
    for (int j = 0; j < JW; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        Pb[(int64_t)(16 * n + 4 * lk + i) * K2 + 16 * (w * JW + j) + li] = acc[n][j][i];
}

// ---------------------------------------------------------------- host side
// mirec_ngcf_grid_cap: most workgroups K16a / K16b launch (0: the CUs decide)
static GridCap g_ng_cap;

// workgroups that give every wave one 16-row slab of M rows
static int64_t ng_groups(int64_t M) { return ((M + 15) / 16 + kNgWaves - 1) / kNgWaves; }

static RowsLd ng_rows(const mirec_rows_ld* a) {
  if (!a) return RowsLd{nullptr, nullptr, 0, 0};
  return RowsLd{a->lo, a->hi ? a->hi : a->lo, a->hi ? a->split : INT64_MAX, a->ld};
}

// every row of a rows operand is read as float4s at a multiple of 16 columns
static bool ng_rows_ok(const mirec_rows_ld* a, int d) {
  return a && a->lo && a->ld >= d && (a->ld % 4) == 0 && ((uintptr_t)a->lo % 16) == 0 &&
         ((uintptr_t)a->hi % 16) == 0 && (!a->hi || a->split >= 0);
}

// K16a / K16b run persistent grids of as many workgroups as a CU holds (prepare_launch: two
// for the 64 -> 64 backward, one for the wide forms).
template <int DI, int DO, bool DROP>
static int launch_fwd(const RowsLd& E, const float* x, int64_t M, const float* W1, const float* b1,
                      const float* W2, const float* b2, const RowsLd& out, float* copy, float* nrm,
                      const DropSite& dr, hipStream_t st, const char* what) {
  constexpr size_t lds = (size_t)DO * (2 * DI + 4) * sizeof(float);
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(ngcf_fwd_kernel<DI, DO, DROP>, kNgThreads, lds, cache, &per_cu, what))
    return -1;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((ngcf_fwd_kernel<DI, DO, DROP>), dim3(g_ng_cap.grid(ng_groups(M), most)),
                     dim3(kNgThreads), lds, st, E, x, M, W1, b1, W2, b2, out, copy, nrm, dr);
  return launch_status(what);
}

template <int DI, int DO, bool DROP>
static int launch_bwd(const RowsLd& G, const RowsLd& En, const float* nrm, int64_t M,
                      const float* W1, const float* W2, const RowsLd& El, const float* x,
                      const RowsLd& add, float* gz, float* dE, float* gx, const DropSite& dr,
                      hipStream_t st, const char* what) {
  constexpr size_t lds = (size_t)2 * DI * (DO + 4) * sizeof(float);
  static int cache[kMaxDev] = {};
  int per_cu = 1;
  if (prepare_launch(ngcf_bwd_kernel<DI, DO, DROP>, kNgThreads, lds, cache, &per_cu, what))
    return -1;
  const int64_t most = (int64_t)device_cus(current_device()) * per_cu;
  hipLaunchKernelGGL((ngcf_bwd_kernel<DI, DO, DROP>), dim3(g_ng_cap.grid(ng_groups(M), most)),
                     dim3(kNgThreads), lds, st, G, En, nrm, M, W1, W2, El, x, add, gz, dE, gx, dr);
  return launch_status(what);
}

constexpr int64_t kNgWgradRows = 256;     // least rows per K16c block
constexpr int kNgWgradMax = 512;          // most partials

// K16c's row split: a block's rows are a multiple of the 16 it loads at a time
static RowSplit ng_wgrad_split(int64_t n) {
  return row_split(n, kNgWgradMax, 16, kNgWgradRows);
}

static int ngcf_shape_error(const char* what, int32_t d_in, int32_t d_out) {
  set_error("%s: widths %d -> %d not in the built set ({64,128}^2)", what, d_in, d_out);
  return -1;
}

}  // namespace mirec

using namespace mirec;

#define MIREC_NG_WIDTHS(F) F(64, 64) F(64, 128) F(128, 64) F(128, 128)

extern "C" int32_t mirec_ngcf_grid_cap(int32_t workgroups) {
  return g_ng_cap.exchange(workgroups);
}

extern "C" int mirec_ngcf_shape_ok(int32_t d_in, int32_t d_out) {
  return (d_in == 64 || d_in == 128) && (d_out == 64 || d_out == 128);
}

extern "C" int mirec_ngcf_layer_fwd_f32(const mirec_rows_ld* E, const float* x, int64_t n,
                                        int32_t d_in, int32_t d_out, const float* W1,
                                        const float* b1, const float* W2, const float* b2,
                                        const mirec_rows_ld* out, float* copy, float* nrm, float p,
                                        uint64_t seed, int64_t* counter, int64_t* drawn,
                                        void* stream) {
  const char* what = "mirec_ngcf_layer_fwd_f32";
  if (!mirec_ngcf_shape_ok(d_in, d_out)) return ngcf_shape_error(what, d_in, d_out);
  if (n < 0 || !ng_rows_ok(E, d_in) || !ng_rows_ok(out, d_out) || !x || !W1 || !b1 || !W2 || !b2 ||
      !nrm || (((uintptr_t)x | (uintptr_t)W1 | (uintptr_t)W2) & 15)) {
    set_error("%s: bad arguments (16-byte aligned rows, x, W1, W2; ld >= width, ld %% 4 == 0)",
              what);
    return -1;
  }
  DropSite dr;
  if (drop_site_or_off(p, seed, counter, drawn, &dr, what)) return -1;
  if (n == 0) return 0;
  const RowsLd e = ng_rows(E), o = ng_rows(out);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_NG(DI, DO)                                                                        \
  if (d_in == DI && d_out == DO)                                                                \
    return p > 0.f ? launch_fwd<DI, DO, true>(e, x, n, W1, b1, W2, b2, o, copy, nrm, dr, st, what) \
                   : launch_fwd<DI, DO, false>(e, x, n, W1, b1, W2, b2, o, copy, nrm, dr, st, what);
  MIREC_NG_WIDTHS(MIREC_NG)
#undef MIREC_NG
  return -1;
}

extern "C" int mirec_ngcf_layer_bwd_f32(const mirec_rows_ld* G, const mirec_rows_ld* E_next,
                                        const float* nrm, int64_t n, int32_t d_in, int32_t d_out,
                                        const float* W1, const float* W2, const mirec_rows_ld* E,
                                        const float* x, const mirec_rows_ld* add, float* gz,
                                        float* dE, float* gx, float p, uint64_t seed,
                                        int64_t* drawn, int64_t* counter, void* stream) {
  const char* what = "mirec_ngcf_layer_bwd_f32";
  if (!mirec_ngcf_shape_ok(d_in, d_out)) return ngcf_shape_error(what, d_in, d_out);
  if (n < 0 || !ng_rows_ok(G, d_out) || !ng_rows_ok(E_next, d_out) || !ng_rows_ok(E, d_in) ||
      (add && add->lo && !ng_rows_ok(add, d_in)) || !nrm || !x || !W1 || !W2 || !gz || !dE || !gx ||
      (((uintptr_t)x | (uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)gz) & 15)) {
    set_error("%s: bad arguments (16-byte aligned rows, x, W1, W2, gz; ld >= width, ld %% 4 == 0)",
              what);
    return -1;
  }
  DropSite dr;
  if (drop_site_or_off(p, seed, counter, drawn, &dr, what)) return -1;
  if (n == 0) return 0;
  const RowsLd g = ng_rows(G), en = ng_rows(E_next), el = ng_rows(E),
               ad = ng_rows(add && add->lo ? add : nullptr);
  hipStream_t st = (hipStream_t)stream;
#define MIREC_NG(DI, DO)                                                                        \
  if (d_in == DI && d_out == DO)                                                                \
    return p > 0.f ? launch_bwd<DI, DO, true>(g, en, nrm, n, W1, W2, el, x, ad, gz, dE, gx, dr, \
                                              st, what)                                         \
                   : launch_bwd<DI, DO, false>(g, en, nrm, n, W1, W2, el, x, ad, gz, dE, gx, dr, \
                                               st, what);
  MIREC_NG_WIDTHS(MIREC_NG)
#undef MIREC_NG
  return -1;
}

extern "C" int32_t mirec_ngcf_wgrad_splits(int64_t n) {
  if (n <= 0) return 0;
  return ng_wgrad_split(n).splits;
}

extern "C" int mirec_ngcf_wgrad_f32(const float* gz, const mirec_rows_ld* E, const float* x,
                                    int64_t n, int32_t d_in, int32_t d_out, float* partials,
                                    void* stream) {
  const char* what = "mirec_ngcf_wgrad_f32";
  if (!mirec_ngcf_shape_ok(d_in, d_out)) return ngcf_shape_error(what, d_in, d_out);
  if (n <= 0 || !gz || !x || !partials || !ng_rows_ok(E, d_in)) {
    set_error("%s: bad arguments", what);
    return -1;
  }
  const RowsLd e = ng_rows(E);
  const RowSplit sp = ng_wgrad_split(n);
#define MIREC_NG(DI, DO)                                                                     \
  if (d_in == DI && d_out == DO)                                                             \
    hipLaunchKernelGGL((ngcf_wgrad_kernel<DI, DO>), dim3((unsigned)sp.splits),              \
                       dim3(kNgThreads), 0, (hipStream_t)stream, gz, e, x, n, sp.rows, partials);
  MIREC_NG_WIDTHS(MIREC_NG)
#undef MIREC_NG
  return launch_status(what);
}
