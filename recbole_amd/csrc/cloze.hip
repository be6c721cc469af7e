// K17 — BERT4Rec's Cloze task on the device: the masking of a training batch, the
// compaction of its loss rows and the placement of their gradients. No host work, no host
// synchronisation; every launch size is known on the host. numpy restatement:
// tests/cloze_spec.py.
//
// K17a cloze_mask: restates BERT4Rec.reconstruct_train_data (bert4rec.py:111-156), which
//   copies the batch to the host and loops over every position in Python. One wave per
//   sequence (L <= 64), lane t holds item_seq[b][t].
//   Mask draw (drop.h): key = drop_key(seed, c), c the site's device counter, which the
//   kernel only READS (a forward without a backward: the caller advances it by one after
//   the launch). Element e = b*L + t with item > 0 is masked iff
//   !drop_keep(key, e, drop_threshold(mask_ratio)).
//   Outputs, the reference's four tensors in its layout: masked_seq[B, L] (a masked
//   position holds mask_token = n_items), pos_items / masked_index / neg_items [B, M], left
//   padded with 0; a row with more than M masked positions keeps the LAST M
//   (_padding_sequence). Rank of a masked lane among its row's = popcount of the ballot
//   below the lane: no atomics. neg_items null: not drawn.
//   Negative of masked element e (only of the kept slots): attempts k = 0, 1, ... take
//     w_k  = mix64(mix64(key ^ 2^63 ^ e) + k)          (e < 2^63: no mask draw's word)
//     cand = 1 + (((w_k >> 32) * (n_items - 1)) >> 32)  in [1, n_items - 1]
//   and the first cand that equals none of the row's L ORIGINAL entries is kept. The wave
//   walks its kept masked lanes in ascending order and tests each attempt with one ballot
//   over the lanes' items. After kClozeAttempts rejected attempts (probability below
//   (64/65)^4096 < 1e-27 for any catalogue the host admits, n_items - 1 > L) the smallest
//   id >= 1 not in the row is taken, so the loop is bounded whatever the data.
//
// K17b cloze_compact: one workgroup walks the [B, M] slots in ascending (b, slot) order,
//   256 at a time, and keeps those with masked_index > 0 (the reference's targets =
//   (masked_index > 0), which also drops a genuinely masked position 0) by a block scan in
//   a fixed order: act_row = b*L + index (a row of the [B*L, d] encoder output), act_target
//   = pos_items, slot_of[b*L + index] = the compact row, -1 for every other position;
//   n_act on the device; act_row / act_target past n_act are 0. No atomics.
//
// K17c rows_from_slots: gX[p] = gS[slot_of[p]] where slot_of[p] >= 0, exact zeros
//   elsewhere; every element of gX written once (no zero fill, no index_add_).
#include "common.h"
#include "drop.h"

namespace mirec {

constexpr int kClozeAttempts = 4096;

__global__ __launch_bounds__(256) void cloze_mask_kernel(
    const int64_t* __restrict__ seq, int64_t B, int L, int M, int64_t n_items, uint32_t thr,
    uint64_t seed, const int64_t* __restrict__ counter, int64_t* __restrict__ masked_seq,
    int64_t* __restrict__ pos_items, int64_t* __restrict__ masked_index,
    int64_t* __restrict__ neg_items) {
  const int t = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                  // wave-uniform
  const uint64_t key = drop_key(seed, counter[0]);
  const bool in = t < L;
  const int64_t item = in ? seq[b * L + t] : 0;
  const uint64_t e = (uint64_t)(b * L + t);
  const bool masked = in && item > 0 && !drop_keep(key, e, thr);
  const uint64_t bal = __ballot(masked);
  const int total = __popcll(bal);
  const int rank = __popcll(bal & ((1ull << t) - 1ull));
  const int slot = M - total + rank;                   // < 0: truncated away
  if (in) masked_seq[b * L + t] = masked ? n_items : item;
  if (t < M - total) {                                 // the left padding
    pos_items[b * M + t] = 0;
    masked_index[b * M + t] = 0;
    if (neg_items) neg_items[b * M + t] = 0;
  }
  const bool kept = masked && slot >= 0;
  if (kept) {
    pos_items[b * M + slot] = item;
    masked_index[b * M + slot] = t;
  }
  if (!neg_items) return;
  uint64_t todo = __ballot(kept);
  while (todo) {                                       // wave-uniform loop
    const int src = __ffsll((unsigned long long)todo) - 1;
    todo &= todo - 1;
    const uint64_t es = (uint64_t)(b * L + src);
    const uint64_t base = mix64(key ^ 0x8000000000000000ull ^ es);
    int64_t cand = 0;
    bool found = false;
    for (int k = 0; k < kClozeAttempts; ++k) {
      const uint64_t w = mix64(base + (uint64_t)k);
      cand = 1 + (int64_t)(((w >> 32) * (uint64_t)(n_items - 1)) >> 32);
      if (__ballot(in && item == cand) == 0) {
        found = true;
        break;
      }
    }
    if (!found) {
      for (cand = 1; cand < n_items; ++cand)        // more than L ids: one is free
        if (__ballot(in && item == cand) == 0) break;
    }
    if (t == src) neg_items[b * M + slot] = cand;
  }
}

__global__ __launch_bounds__(256) void cloze_compact_kernel(
    const int64_t* __restrict__ masked_index, const int64_t* __restrict__ pos_items, int64_t B,
    int L, int M, int64_t* __restrict__ act_row, int64_t* __restrict__ act_target,
    int32_t* __restrict__ n_act, int32_t* __restrict__ slot_of) {
  __shared__ int lds[8];
  const int64_t n_pos = B * L, n_slot = B * M;
  for (int64_t p = threadIdx.x; p < n_pos; p += 256) slot_of[p] = -1;
  __syncthreads();                                     // the -1s land before the live slots
  int base = 0;
  for (int64_t s0 = 0; s0 < n_slot; s0 += 256) {       // uniform trip count
    const int64_t s = s0 + threadIdx.x;
    const int64_t idx = s < n_slot ? masked_index[s] : 0;
    const int flag = (idx > 0 && idx < L) ? 1 : 0;    // K17a writes no index >= L
    int total;
    const int at = base + block_exclusive_scan(flag, lds, &total);
    if (flag) {
      const int64_t p = (s / M) * L + idx;
      act_row[at] = p;
      act_target[at] = pos_items[s];
      slot_of[p] = at;
    }
    base += total;
  }
  for (int64_t s = base + threadIdx.x; s < n_slot; s += 256) {
    act_row[s] = 0;
    act_target[s] = 0;
  }
  if (threadIdx.x == 0) n_act[0] = base;
}

__global__ __launch_bounds__(256) void rows_from_slots_kernel(
    const float4* __restrict__ gS, const int32_t* __restrict__ slot_of, int64_t n_pos, int d4,
    float4* __restrict__ gX) {
  const int64_t n = n_pos * d4;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p = e / d4;
    const int c = (int)(e - p * d4);
    const int s = slot_of[p];
    gX[e] = s >= 0 ? gS[(int64_t)s * d4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

}  // namespace mirec

using namespace mirec;

extern "C" int mirec_cloze_mask(const int64_t* item_seq, int64_t B, int32_t L, int32_t M,
                                int64_t n_items, double mask_ratio, uint64_t seed,
                                const int64_t* counter, int64_t* masked_seq,
                                int64_t* pos_items, int64_t* masked_index, int64_t* neg_items,
                                void* stream) {
  if (B == 0) return 0;
  if (!item_seq || !counter || !masked_seq || !pos_items || !masked_index || B < 0 || L < 1 ||
      L > 64 || M < 1 || M > L || !(mask_ratio > 0.0 && mask_ratio < 1.0)) {
    set_error("mirec_cloze_mask: bad arguments (1 <= M <= L <= 64, 0 < mask_ratio < 1)");
    return -1;
  }
  if (n_items - 1 <= L) {
    set_error("mirec_cloze_mask: n_items - 1 = %lld <= L = %d (a negative could not be drawn)",
              (long long)(n_items - 1), L);
    return -1;
  }
  hipLaunchKernelGGL(cloze_mask_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0,
                     (hipStream_t)stream, item_seq, B, L, M, n_items,
                     drop_threshold(mask_ratio), seed, counter, masked_seq, pos_items,
                     masked_index, neg_items);
  return launch_status("mirec_cloze_mask");
}

extern "C" int mirec_cloze_compact(const int64_t* masked_index, const int64_t* pos_items,
                                   int64_t B, int32_t L, int32_t M, int64_t* act_row,
                                   int64_t* act_target, int32_t* n_act, int32_t* slot_of,
                                   void* stream) {
  if (!n_act) {
    set_error("mirec_cloze_compact: bad arguments");
    return -1;
  }
  if (B > 0 && (!masked_index || !pos_items || !act_row || !act_target || !slot_of || L < 1 ||
                M < 1 || B * (int64_t)L > INT32_MAX || B * (int64_t)M > INT32_MAX)) {
    set_error("mirec_cloze_compact: bad arguments (B * L and B * M must fit int32)");
    return -1;
  }
  hipLaunchKernelGGL(cloze_compact_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream,
                     masked_index, pos_items, B < 0 ? 0 : B, L, M, act_row, act_target, n_act,
                     slot_of);
  return launch_status("mirec_cloze_compact");
}

extern "C" int mirec_rows_from_slots_f32(const float* gS, const int32_t* slot_of, int64_t n_pos,
                                         int32_t d, float* gX, void* stream) {
  if (n_pos == 0) return 0;
  if (!gS || !slot_of || !gX || n_pos < 0 || d < 4 || d % 4) {
    set_error("mirec_rows_from_slots_f32: bad arguments (d a multiple of 4)");
    return -1;
  }
  const int64_t g = (n_pos * (d / 4) + 255) / 256;
  hipLaunchKernelGGL(rows_from_slots_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256),
                     0, (hipStream_t)stream, (const float4*)gS, slot_of, n_pos, d / 4,
                     (float4*)gX);
  return launch_status("mirec_rows_from_slots_f32");
}
