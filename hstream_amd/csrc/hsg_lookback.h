// The ordered compaction's tile protocol, device side: a chained scan with
// look-back over tile states. Every pass that compacts kept rows in order goes
// through here. A tile's state is one 8-byte word, status and count together,
// moved by relaxed agent-scope atomics, so there is no payload to order behind
// a flag:
//   0                 nothing published yet
//   kStAgg | count    the tile's own kept count
//   kStSum | sum      the kept count of tiles [0, t], the tile's included
// Tiles are handed out in order by a ticket, so a tile only ever waits for
// tiles already taken. Polling is bounded: a tile that waits past kMaxPolls
// sets the caller's error bit and gives up, and the push fails instead of
// hanging.
//
// A workgroup's loop over tiles is take_tile, the pass's own loads and
// verdicts, rank_kept, publish_tile, the pass's own writes at the offset, and
// a workgroup barrier before the next take_tile (TileLds is reused).
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
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
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

// The workgroup's LDS of the protocol, W waves of one row per thread.
template <int W>
struct TileLds {
  uint32_t wcnt[W];
  uint64_t tile, excl;
};

// The next tile of the launch, to the whole workgroup: state[0] is the ticket
// (zeroed before the launch). A ticket past the last tile ends the workgroup.
template <int W>
__device__ __forceinline__ uint64_t take_tile(TileLds<W> &s, uint64_t *state) {
  if (threadIdx.x == 0) s.tile = atomicAdd((unsigned long long *)state, 1ull);
  __syncthreads();
  return s.tile;
}

// This lane's rank among the tile's kept rows (wave ballots, a scan of the
// wave counts in LDS) and the tile's kept count.
struct Rank {
  uint32_t rank, count;
};
template <int W>
__device__ __forceinline__ Rank rank_kept(TileLds<W> &s, bool keep) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  if (lane == 0) s.wcnt[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  uint32_t before = 0, count = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) {
    before += w < wave ? s.wcnt[w] : 0;
    count += s.wcnt[w];
  }
  return {before + (uint32_t)__popcll(m & ((1ull << lane) - 1)), count};
}

// Tile t of n_tiles kept `count` rows: wave 0 publishes the count, looks back
// for the rows kept before the tile, and publishes the inclusive sum; the last
// tile leaves `ran | total` in *total_word for the host. To the whole
// workgroup: the tile's exclusive offset, or kNoSum (uniform; the workgroup
// then writes nothing and takes no further tile). tiles = state + 2.
template <int W>
__device__ __forceinline__ uint64_t publish_tile(TileLds<W> &s, uint64_t *tiles, uint64_t t, uint64_t n_tiles,
                                                 uint32_t count, DevScalars *sc, uint32_t err_bit,
                                                 uint64_t *total_word, uint64_t ran) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    if (lane == 0) st_store(tiles + t, kStAgg | count);
    const uint64_t excl = look_back(tiles, t, sc, err_bit);
    if (lane == 0) {
      s.excl = excl;
      if (excl != kNoSum) {
        st_store(tiles + t, kStSum | (excl + count));
        if (t == n_tiles - 1) *total_word = ran | (excl + count);
      }
    }
  }
  __syncthreads();
  return s.excl;
}

}  // namespace lookback
}  // namespace hsg
