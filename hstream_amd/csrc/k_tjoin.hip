// gfx950 kernels of the stream-table join (hsg_table_join): for each record of
// a poll batch, in arrival order, the row an unwindowed op's table holds for
// the record's key. What it replaces is the reference's joinTableProcessor
// (hstream-processing/src/HStream/Processing/Stream.hs:302-344): ksGet of the
// record's key in the table's KV store, a forward on a hit, nothing on a miss.
// The store is what GroupedStream.aggregate returns (GroupedStream.hs:53-56),
// here the unwindowed op's HBM table (hsg_tw.h).
//
// Find pass -> exclusive scan of the tiles' hit counts -> rows pass, as the
// keyed view read (k_view.hip): no workgroup waits for another inside a
// launch, a row's position depends only on the batch and the table, and the
// host reads the total between the passes (the capacity rule of hsg_drain).
// A workgroup takes a tile of kTjTile consecutive records, thread t the
// records t, t + 256, ... of it, so key loads, slot words and, over the
// tile's hits, the column stores are coalesced.
//
// An unwindowed table never spills closed windows to the host (retention.cpp
// tw_maintain counts closed windows only where window_kind != HSG_UNWINDOWED:
// the one implicit window never closes), so unlike the keyed view read there
// is deliberately no merge with spilled rows here.
#include "hsg_dev.h"
#include "hsg_kernels.h"
#include "hsg_sort.h"
#include "hsg_tw.h"

namespace hsg {

constexpr int kTjThreads = 256;
constexpr int kTjPer = 4;  // records per thread: home-slot loads in flight per lane
static_assert(kTjThreads * kTjPer == kTjTile, "tile");
static_assert(kTjThreads == 256, "four waves: the LDS sums below");

// Record (r, thread) of the tile is tile * kTjTile + r * 256 + thread. The pass
// is bound by random HBM round trips, one per record: a thread issues the
// home-slot key loads of its kTjPer records before it looks at any of them;
// only a displaced key (its home slot holds another group) probes on, with
// tw_find's own continuation (other slots of the region, then the overflow
// rows). HSG_KEY_NONE and the records past n miss.
__global__ __launch_bounds__(kTjThreads) void k_tjoin_find(TwTable t, const uint32_t *__restrict__ keys, uint64_t n,
                                                           int64_t *__restrict__ slot, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t sw[kTjThreads / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kTjTile + threadIdx.x;
  uint32_t key[kTjPer];
  uint64_t home[kTjPer], cur[kTjPer];
  // branch-free up to the probe, so nothing waits between the loads: a record
  // past n reads the batch's last key (n > 0) and a keyless one the home slot
  // its id hashes to, which is inside the table like any other
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    const uint64_t i = i0 + (uint64_t)r * kTjThreads;
    key[r] = keys[i < n ? i : n - 1];
  }
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    home[r] = tw_home(t, (uint64_t)key[r] << 32);  // the one implicit window: k = 0, epoch 0
    cur[r] = *t.key(home[r]);
  }
  uint32_t h = 0;  // the wave's hits (uniform)
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    const uint64_t i = i0 + (uint64_t)r * kTjThreads;
    const bool probe = i < n && key[r] != HSG_KEY_NONE;
    const int64_t s = probe ? tw_find_from(t, (uint64_t)key[r] << 32, home[r], cur[r]) : -1;
    if (i < n) slot[i] = s;
    h += (uint32_t)__popcll(__ballot(s >= 0));
  }
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

// A hit's output row is the tile's offset plus the hits before it in the tile
// in arrival order: the hits of rounds before r, of the waves before w in
// round r (both through LDS), and of the lanes below it in its wave's ballot.
// Null output columns (the caller does not want them) are skipped.
__global__ __launch_bounds__(kTjThreads) void k_tjoin_rows(TwTable t, Program prog, const uint32_t *__restrict__ keys,
                                                           uint64_t n, const int64_t *__restrict__ slot,
                                                           const uint64_t *__restrict__ off, OutCols out,
                                                           uint64_t out_cap) {
  __shared__ uint32_t sw[kTjPer][kTjThreads / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t i0 = (uint64_t)blockIdx.x * kTjTile + threadIdx.x;
  int64_t s[kTjPer];
  uint64_t mask[kTjPer];
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    const uint64_t i = i0 + (uint64_t)r * kTjThreads;
    s[r] = i < n ? slot[i] : -1;
  }
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    mask[r] = __ballot(s[r] >= 0);
    if (lane == 0) sw[r][w] = (uint32_t)__popcll(mask[r]);
  }
  __syncthreads();
  uint64_t run = off[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kTjPer; ++r) {
    uint64_t o = run + (uint64_t)__popcll(mask[r] & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) o += sw[r][k];
    run += sw[r][0] + sw[r][1] + sw[r][2] + sw[r][3];
    if (s[r] < 0 || o >= out_cap) continue;
    const uint64_t i = i0 + (uint64_t)r * kTjThreads;
    const int64_t *row = t.aggs((uint64_t)s[r]);
    if (out.key) out.key[o] = keys[i];
    if (out.ws) out.ws[o] = 0;
    if (out.we) out.we[o] = 0;
    if (out.src) out.src[o] = (int64_t)i;
    for (int j = 0; j < prog.n_out; ++j)
      if (out.agg[j]) out.agg[j][o] = out_value(prog, j, row);
    if (out.form) out.form[o] = out_form(prog, row);
  }
}

void launch_tjoin_find(hipStream_t s, const TwTable &t, const uint32_t *keys, uint64_t n, int64_t *slot,
                       const EmitScratch &es, uint64_t *total) {
  const uint64_t tiles = tjoin_tiles(n);
  hipLaunchKernelGGL(k_tjoin_find, dim3((unsigned)tiles), dim3(kTjThreads), 0, s, t, keys, n, slot, es.cnt);
  scan_excl_u32(s, es.cnt, es.off, tiles, es.partial, total);
}

void launch_tjoin_rows(hipStream_t s, const TwTable &t, const Program &prog, const uint32_t *keys, uint64_t n,
                       const int64_t *slot, const EmitScratch &es, OutCols out, uint64_t out_cap) {
  hipLaunchKernelGGL(k_tjoin_rows, dim3((unsigned)tjoin_tiles(n)), dim3(kTjThreads), 0, s, t, prog, keys, n, slot,
                     es.off, out, out_cap);
}

}  // namespace hsg
