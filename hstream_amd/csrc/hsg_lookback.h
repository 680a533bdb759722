// The chained scan's look-back over tile states, device side: the protocol of
// the ordered compactions (k_having.hip over a changelog segment, k_select.hip
// over a staged batch). A tile's state is one 8-byte word, status and count
// together, moved by relaxed agent-scope atomics, so there is no payload to
// order behind a flag:
//   0                 nothing published yet
//   kStAgg | count    the tile's own kept count
//   kStSum | sum      the kept count of tiles [0, t], the tile's included
// Tiles are handed out in order by a ticket, so a tile only ever waits for
// tiles already taken. Polling is bounded: a tile that waits past kMaxPolls
// sets the caller's error bit and gives up, and the push fails instead of
// hanging.
#pragma once

#include "hsg_internal.h"

namespace hsg {
namespace lookback {

constexpr uint64_t kStAgg = 1ull << 62, kStSum = 2ull << 62, kStMask = 3ull << 62;
// polls of a predecessor before a tile gives up: a tile's work is tens of
// microseconds, a poll about one
constexpr uint32_t kMaxPolls = 1u << 20;
// look_back's answer then: the tile has no offset, so it writes no row and
// publishes no sum, and its workgroup takes no further tile (the tiles behind
// it give up the same way; the push fails with the error bit and counts no row)
constexpr uint64_t kNoSum = ~0ull;

__device__ __forceinline__ uint64_t st_load(const uint64_t *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_store(uint64_t *p, uint64_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Wave 0 of tile t: the kept rows of tiles [0, t). Lane l reads the state of
// tile t - 1 - l (64 predecessors a round); the round ends at the nearest
// inclusive sum once every tile between it and t has published. err_bit: the
// DevScalars::err bit of the pass (ERR_HAVING, ERR_SELECT).
__device__ __forceinline__ uint64_t look_back(const uint64_t *tiles, uint64_t t, DevScalars *sc, uint32_t err_bit) {
  const int lane = threadIdx.x & 63;
  uint64_t excl = 0;
  uint64_t hi = t;  // this round reads tiles hi - 1 - lane
  uint32_t polls = 0;
  while (true) {
    const bool real = (uint64_t)lane < hi;
    // before tile 0: an inclusive sum of 0
    const uint64_t w = real ? st_load(tiles + (hi - 1 - lane)) : kStSum;
    const uint64_t stat = w & kStMask;
    const uint64_t sums = __ballot(stat == kStSum);
    const int first = sums ? __builtin_ctzll(sums) : 64;
    const uint64_t need = first >= 63 ? ~0ull : ((2ull << first) - 1);
    const uint64_t missing = __ballot(stat == 0) & need;
    if (missing) {
      if (++polls > kMaxPolls) {
        if (lane == 0) atomicOr(&sc->err, err_bit);
        return kNoSum;
      }
      __builtin_amdgcn_s_sleep(2);
      continue;
    }
    excl += wave_sum(lane <= first ? (w & ~kStMask) : 0);
    if (first < 64) return excl;
    hi -= 64;
  }
}

}  // namespace lookback
}  // namespace hsg
