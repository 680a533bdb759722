// Device helpers shared by the gfx950 kernels (wave64 scans / reductions,
// output conversion; the aggregate-slot algebra is hsg_slots.h). Not part of
// the ABI.
#pragma once

#include "hsg_internal.h"
#include "hsg_part.h"
#include "hsg_slots.h"

namespace hsg {

// Phase clocks of the HSG_PHASES diagnostics (per-workgroup time split of the
// partition, aggregation, per-record and session kernels, summed into
// DevScalars::scratch and printed by op_device.cpp). Compiled in only with
// -DHSG_PHASE_CLOCKS=1 (make PHASES=1): otherwise phase_clock() is 0 and every
// accumulation guarded by kPhaseClocks is dead code, so the product kernels
// carry neither the clock reads nor the atomics.
#ifndef HSG_PHASE_CLOCKS
#define HSG_PHASE_CLOCKS 0
#endif
constexpr bool kPhaseClocks = HSG_PHASE_CLOCKS != 0;
__device__ inline uint64_t phase_clock() {
  if constexpr (kPhaseClocks) return wall_clock64();
  return 0;
}

__device__ inline int64_t wave_max_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int64_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ inline int64_t wave_min_i64(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    int64_t u = __shfl_xor(v, o, 64);
    v = u < v ? u : v;
  }
  return v;
}
__device__ inline uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ inline int64_t wave_incl_max(int64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int64_t u = __shfl_up(v, o, 64);
    if (lane >= o) v = u > v ? u : v;
  }
  return v;
}
__device__ inline uint64_t wave_incl_sum(uint64_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint64_t u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// Workgroup barrier that orders LDS only: __syncthreads() also waits for the
// wave's outstanding global stores (its workgroup-scope release), which costs
// microseconds after a burst of scattered stores that no one in the workgroup
// reads back. Use where the only data crossing the barrier is in LDS.
__device__ inline void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// a form slot's word for a present record: (seq + 1) << 1 | integral literal
__device__ inline int64_t form_word(const Batch &b, int c, uint64_t i, uint64_t seq1) {
  return (int64_t)((seq1 << 1) | (rec_decimal(b, c, i) ? 0u : 1u));
}

// Sequence word of a partitioned record of an op with LAST / literal-form
// slots (hsg_part.h): (global seq + 1) in the low 56 bits, bit 56 + c set when
// column c's literal is decimal (bit 1 of its valid byte).
__device__ inline uint64_t seq_word(const Batch &b, int C, int has_valid, int64_t seq, uint64_t i) {
  uint64_t w = (uint64_t)(seq + 1) & kSeqMask;
  if (has_valid)
    for (int c = 0; c < C && c < 8; ++c)
      if (b.valid[c] && (b.valid[c][i] & 2u)) w |= 1ull << (56 + c);
  return w;
}

__device__ inline int64_t out_value_w(const Program &prog, int j, int64_t a, int64_t bcnt) {
  switch (prog.out_kind[j]) {
    case O_F64_ORD: return __builtin_bit_cast(int64_t, f64_unord((uint64_t)a));
    case O_AVG_I: {
      double d = bcnt ? (double)a / (double)bcnt : __builtin_nan("");
      return __builtin_bit_cast(int64_t, d);
    }
    case O_AVG_F: {
      double d = bcnt ? __builtin_bit_cast(double, a) / (double)bcnt : __builtin_nan("");
      return __builtin_bit_cast(int64_t, d);
    }
    default: return a;
  }
}

// XCD-aware tile order: workgroups are dealt round-robin over the 8 XCDs, so
// give workgroups b, b+8, b+16, ... (one XCD) consecutive tiles; a bucket's
// runs from consecutive tiles are adjacent in the output. Speed only.
__device__ inline uint64_t xcd_tile(uint64_t blk, uint64_t tiles) {
  const uint64_t per = tiles / 8, full = per * 8;
  if (blk >= full) return blk;
  return (blk & 7) * per + (blk >> 3);
}

// output column j from a state row in memory
__device__ inline int64_t out_value(const Program &prog, int j, const int64_t *row) {
  return out_value_w(prog, j, row[prog.out_a[j]], row[prog.out_b[j]]);
}

template <int MS>
__device__ inline int64_t out_value_reg(const Program &prog, int j, const int64_t (&r)[MS]) {
  int64_t a = 0, b = 0;
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    if (s == prog.out_a[j]) a = r[s];
    if (s == prog.out_b[j]) b = r[s];
  }
  return out_value_w(prog, j, a, b);
}

// Literal forms of a row's outputs (hsg_rows.form; hsg_internal.h FormKind):
// bit 2j = output j prints as an integer, bit 2j + 1 = it is the aggregate's
// initial value. fa = the output's form slot.
__device__ inline uint32_t form_bits_w(int kind, int64_t fa) {
  switch (kind) {
    case F_SUM: return fa == 0 ? 1u : 0u;
    case F_MIN: return fa == 1 ? 3u : (uint32_t)(fa & 1);
    case F_MAX:
    case F_LAST: return fa == 0 ? 3u : (uint32_t)(fa & 1);
    default: return 0u;
  }
}
__device__ inline uint32_t out_form(const Program &prog, const int64_t *row) {
  uint32_t f = 0;
  for (int j = 0; j < prog.n_out; ++j)
    if (prog.form_kind[j] != F_NONE) f |= form_bits_w(prog.form_kind[j], row[prog.form_a[j]]) << (2 * j);
  return f;
}
template <int MS>
__device__ inline uint32_t out_form_reg(const Program &prog, const int64_t (&r)[MS]) {
  uint32_t f = 0;
  for (int j = 0; j < prog.n_out; ++j)
    if (prog.form_kind[j] != F_NONE) f |= form_bits_w(prog.form_kind[j], reg_at<MS>(r, prog.form_a[j])) << (2 * j);
  return f;
}

// Per-record stream time for the records of one tile (record (r, thread) =
// tile_base + r*kTileThreads + thread), inclusive prefix max in arrival order
// seeded with the tile's exclusive prefix. Block-wide: every thread must call.
__device__ inline void tile_stream_time(const int64_t (&ts)[kRecPerThread], int64_t carry,
                                        int64_t (&wm)[kRecPerThread]) {
  __shared__ int64_t swave[kTileThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < kRecPerThread; ++r) {
    int64_t incl = wave_incl_max(ts[r]);
    if (lane == 63) swave[w] = incl;
    __syncthreads();
    int64_t before = carry;
    for (int k = 0; k < w; ++k) before = swave[k] > before ? swave[k] : before;
    wm[r] = incl > before ? incl : before;
    int64_t tot = carry;
    for (int k = 0; k < kTileThreads / 64; ++k) tot = swave[k] > tot ? swave[k] : tot;
    carry = tot;
    __syncthreads();
  }
}

// Window range [k_lo, k_hi] of a record (windowsFor, TimeWindowedStream.hs:105-117);
// returns false when the record has no window (ts < 0).
__device__ inline bool record_windows(const TwParams &p, int64_t ts, uint64_t &k_lo, uint64_t &k_hi) {
  if (p.kind == HSG_UNWINDOWED) {
    k_lo = 0;
    k_hi = 0;
    return true;
  }
  if (ts < 0) return false;
  k_hi = udiv(p.div, (uint64_t)ts);
  if (p.size == p.adv) {  // tumbling: the one window (uniform branch)
    k_lo = k_hi;
    return true;
  }
  int64_t t0 = (int64_t)((uint64_t)ts - (uint64_t)p.size + (uint64_t)p.adv);
  if (t0 < 0) t0 = 0;
  k_lo = udiv(p.div, (uint64_t)t0);
  return true;
}

// t + size + grace <= INT64_MAX (size, grace >= 0), without overflowing: no
// window of a record at or before t has an end + grace that wraps
__device__ inline bool tw_sum_fits(int64_t t, int64_t size, int64_t grace) {
  return grace <= INT64_MAX - size && t <= INT64_MAX - size - grace;
}

// grace check of window k against the record's stream time (TimeWindowedStream.hs:92)
__device__ inline bool window_accepted(const TwParams &p, uint64_t k, int64_t wm) {
  if (p.kind == HSG_UNWINDOWED) return true;
  int64_t ws = (int64_t)(k * (uint64_t)p.adv);
  int64_t we = (int64_t)((uint64_t)ws + (uint64_t)p.size);
  return wm < (int64_t)((uint64_t)we + (uint64_t)p.grace);
}

// The accepted windows of a record, as one run inside its windows [k_lo, k_hi]
// (narrowed in place; `late` counts the refused ones). The leading windows may
// have closed (end + grace <= stream time). The trailing ones may end so high
// that end + grace passes INT64_MAX: the reference's Int64 sum wraps negative
// there and refuses them too. Every kernel that lays a record's windows out
// as a run (partition histogram and scatter, the per-record changelog's
// offsets) takes it from here, so their counts agree. False: none accepted.
__device__ inline bool accepted_run(const TwParams &p, int64_t wm, uint64_t &k_lo, uint64_t &k_hi, uint64_t &late) {
  while (k_lo <= k_hi && !window_accepted(p, k_lo, wm)) {
    ++k_lo;
    ++late;
  }
  if (k_lo > k_hi) return false;
  while (k_hi > k_lo && !window_accepted(p, k_hi, wm)) {
    --k_hi;
    ++late;
  }
  return true;
}

}  // namespace hsg
