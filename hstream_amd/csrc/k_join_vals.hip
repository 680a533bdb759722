// gfx950 kernels of the valued stream-stream join (hsg_join.h, "valued join"):
//   k_jv_append  a batch's value columns -> array-of-struct rows of the arena
//                (coalesced column reads, 16-byte row stores) and the records'
//                handles (their row numbers);
//   k_jv_gather  the pending (this handle, other handle) pairs -> the joined
//                rows as columns: both rows loaded with 16-byte loads issued
//                before the first use, every output array written lane = row.
// One thread per row, the stride a template parameter so that a row lives in
// registers under constant indices (no scratch). The rows are 16-128 bytes:
// the gather is bound by the loads in flight, not by bytes.
#include "hsg_dev.h"
#include "hsg_join.h"

namespace hsg {

#define GRID_LOOP(i, n) \
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < (n); i += (uint64_t)gridDim.x * blockDim.x)

// word k of a row held as S / 2 16-byte pieces (k a compile-time constant after unrolling)
__device__ inline uint64_t jv_word(const uint4 *r, int k) {
  const uint4 q = r[k >> 1];
  return (k & 1) ? ((uint64_t)q.w << 32 | q.z) : ((uint64_t)q.y << 32 | q.x);
}

template <int S>
__global__ __launch_bounds__(256) void k_jv_append(JvAppend a) {
  constexpr int C = S - 1 < kJoinMaxCols ? S - 1 : kJoinMaxCols;  // columns a row of this stride can hold
  GRID_LOOP(i, a.n) {
    const int nc = a.side[i] ? a.nc[1] : a.nc[0];
    uint64_t w[S];
#pragma unroll
    for (int k = 0; k < S; ++k) w[k] = 0;
    uint64_t vw = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c < nc) {
        w[c] = ((const uint64_t *)a.cols[c])[i];
        const uint8_t v = a.valid[c] ? a.valid[c][i] : (uint8_t)1;
        vw |= (uint64_t)v << (8 * c);
      }
    }
#pragma unroll
    for (int k = 0; k <= C; ++k)
      if (k == nc) w[k] = vw;
    uint4 *row = (uint4 *)(a.arena + (a.used + i) * S);
#pragma unroll
    for (int q = 0; q < S / 2; ++q)
      row[q] = make_uint4((uint32_t)w[2 * q], (uint32_t)(w[2 * q] >> 32), (uint32_t)w[2 * q + 1],
                          (uint32_t)(w[2 * q + 1] >> 32));
    a.handle[i] = a.used + i;
  }
}

template <int S>
__global__ __launch_bounds__(256) void k_jv_gather(JvGather g) {
  constexpr int C = S - 1 < kJoinMaxCols ? S - 1 : kJoinMaxCols;
  const int nc0 = g.nc[0], nc1 = g.nc[1];
  GRID_LOOP(i, g.n) {
    uint64_t ha = g.this_h[i], hb = g.other_h[i];
    const int64_t ts = g.ts[i];
    const uint32_t jk = g.jkey[i];
    // (handles are this join's own row numbers; never read past the rows in use)
    ha = ha < g.used ? ha : 0;
    hb = hb < g.used ? hb : 0;
    const uint4 *pa = (const uint4 *)(g.arena + ha * S), *pb = (const uint4 *)(g.arena + hb * S);
    uint4 ra[S / 2], rb[S / 2];
#pragma unroll
    for (int q = 0; q < S / 2; ++q) ra[q] = pa[q];
#pragma unroll
    for (int q = 0; q < S / 2; ++q) rb[q] = pb[q];
    uint64_t va = 0, vb = 0;  // the sides' valid bytes
#pragma unroll
    for (int k = 0; k <= C; ++k) {
      if (k == nc0) va = jv_word(ra, k);
      if (k == nc1) vb = jv_word(rb, k);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (c < nc0) {
        if (g.col_a[c]) g.col_a[c][i] = jv_word(ra, c);
        if (g.val_a[c]) g.val_a[c][i] = (uint8_t)(va >> (8 * c));
      }
      if (c < nc1) {
        if (g.col_b[c]) g.col_b[c][i] = jv_word(rb, c);
        if (g.val_b[c]) g.val_b[c][i] = (uint8_t)(vb >> (8 * c));
      }
    }
    if (g.key_id) {
      uint32_t kid = jk;
      if (g.key_col >= 0) {
        const bool in_a = g.key_col < nc0;
        const int k = in_a ? g.key_col : g.key_col - nc0;
        uint64_t v = 0;
#pragma unroll
        for (int c = 0; c < C; ++c)
          if (c == k) v = in_a ? jv_word(ra, c) : jv_word(rb, c);
        const uint32_t present = (uint32_t)((in_a ? va : vb) >> (8 * k)) & 1u;
        kid = present && v <= 0xFFFFFFFEull ? (uint32_t)v : HSG_KEY_NONE;
      }
      g.key_id[i] = kid;
    }
    if (g.o_ts) g.o_ts[i] = ts;
    if (g.o_this) g.o_this[i] = ha;
    if (g.o_other) g.o_other[i] = hb;
    if (g.o_jkey) g.o_jkey[i] = jk;
  }
}

#define JV_LAUNCH(k, n, arg)                                                                               \
  do {                                                                                                     \
    if (n) {                                                                                               \
      const dim3 grid(grid_for(n, 256)), block(256);                                                       \
      if (stride == 2) hipLaunchKernelGGL(k<2>, grid, block, 0, s, arg);                                   \
      else if (stride == 4) hipLaunchKernelGGL(k<4>, grid, block, 0, s, arg);                              \
      else if (stride == 8) hipLaunchKernelGGL(k<8>, grid, block, 0, s, arg);                              \
      else hipLaunchKernelGGL(k<16>, grid, block, 0, s, arg);                                              \
    }                                                                                                      \
  } while (0)

void launch_jv_append(hipStream_t s, const JvAppend &a, uint32_t stride) { JV_LAUNCH(k_jv_append, a.n, a); }
void launch_jv_gather(hipStream_t s, const JvGather &g, uint32_t stride) { JV_LAUNCH(k_jv_gather, g.n, g); }

}  // namespace hsg
