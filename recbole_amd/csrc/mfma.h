// The fp32 MFMA tile every model kernel shares: the accumulator types, the two intrinsics
// and K11's weight-in-LDS slab product (linear.hip; K16 in ngcf.hip and K18 in cin.hip run
// the same loop).
#pragma once
#include <hip/hip_runtime.h>

namespace mirec {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));

// v_mfma_f32_16x16x4_f32: lane (li = lane & 15, lk = lane >> 4) supplies A[li][lk] and
// B[lk][li]; c[i] = C[4 lk + i][li]
__device__ __forceinline__ floatx4 mfma_16x16x4(float a, float b, floatx4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// v_mfma_f32_32x32x2_f32: lane l supplies A[l & 31][l >> 5] and B[l >> 5][l & 31]
__device__ __forceinline__ floatx16 mfma_32x32x2(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// A pointer into LDS that says so in its type. Through a plain (generic) pointer the compiler
// learns that the target is LDS only after inlining and forms the addresses another way;
// neither way is faster everywhere (K11 through a generic pointer: -2 % .. +5 % per shape).
typedef const __attribute__((address_space(3))) float* lds_floats;

__device__ __forceinline__ lds_floats lds_ptr(const float* p) { return (lds_floats)p; }

__device__ __forceinline__ float4 load_float4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ float4 load_float4(lds_floats p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return *(const __attribute__((address_space(3))) float4*)p;
#else
  return float4{};   // the host pass only parses device code (its float4 has no such copy)
#endif
}

// The products of one 16-row slab against a weight held in LDS as Bs[n][k] (row stride KP
// floats): acc[c] = A[:, 16u ..] Bs[16c .., 16u ..]^T summed over the NU k slices u, for the
// NC column tiles c. Lane (li, lk) holds floats 16u + 4lk .. +3 of row li in a[u]. Per
// accumulator the order is u ascending, then x, y, z, w. Bs is a const float* or an
// lds_floats: each caller passes the kind its kernel was tuned and measured with (K11
// lds_ptr(Bs), K16 Bs), which keeps both kernels' instruction streams as they were.
//
// A group g is (k slice u, GA = min(GW, NC) column tiles cg ..). The next group's B reads
// are issued before this group's MFMAs, so their LDS latency passes under the products; the
// GA accumulators are interleaved, so a dependent MFMA follows its predecessor GA issues
// later.
//
// mfma_slab_acc adds the products to acc as it stands (K18's forward walks many weight slabs
// into one set of accumulators); mfma_slab starts from zero.
template <int NU, int NC, int KP, int GW = 4, typename BsPtr>
__device__ __forceinline__ void mfma_slab_acc(const float4 (&a)[NU], BsPtr Bs, int li, int lk,
                                              floatx4 (&acc)[NC]) {
  constexpr int GA = NC < GW ? NC : GW;
  constexpr int NG = NU * (NC / GA);
  static_assert(NC % GA == 0, "the column tiles come in whole groups");
  auto load_b = [&](float4 (&b)[GA], int g) {
    const int u = g / (NC / GA), cg = GA * (g % (NC / GA));
#pragma unroll
    for (int c = 0; c < GA; ++c)
      b[c] = load_float4(&Bs[(16 * (cg + c) + li) * KP + 16 * u + 4 * lk]);
  };
  float4 bc[GA];
  load_b(bc, 0);
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    const int u = g / (NC / GA), cg = GA * (g % (NC / GA));
    float4 bn[GA];
    if (g + 1 < NG) load_b(bn, g + 1);
    __builtin_amdgcn_sched_barrier(0);   // the reads stay ahead of this group's MFMAs
#pragma unroll
    for (int c = 0; c < GA; ++c) acc[cg + c] = mfma_16x16x4(a[u].x, bc[c].x, acc[cg + c]);
#pragma unroll
    for (int c = 0; c < GA; ++c) acc[cg + c] = mfma_16x16x4(a[u].y, bc[c].y, acc[cg + c]);
#pragma unroll
    for (int c = 0; c < GA; ++c) acc[cg + c] = mfma_16x16x4(a[u].z, bc[c].z, acc[cg + c]);
#pragma unroll
    for (int c = 0; c < GA; ++c) acc[cg + c] = mfma_16x16x4(a[u].w, bc[c].w, acc[cg + c]);
    // the scheduler keeps this order (no hoisting of later groups' reads)
    __builtin_amdgcn_sched_barrier(0);
    if (g + 1 < NG)
#pragma unroll
      for (int c = 0; c < GA; ++c) bc[c] = bn[c];
  }
}

template <int NU, int NC, int KP, int GW = 4, typename BsPtr>
__device__ __forceinline__ void mfma_slab(const float4 (&a)[NU], BsPtr Bs, int li, int lk,
                                          floatx4 (&acc)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = floatx4{0.f, 0.f, 0.f, 0.f};
  mfma_slab_acc<NU, NC, KP, GW>(a, Bs, li, lk, acc);
}

}  // namespace mirec
