// HAVING pushdown: the SQL filter over the changelog rows a batch appended.
//
// The reference chains genFilteRNodeFromHaving behind an unwindowed GROUP BY
// (hstream-sql/src/HStream/SQL/Codegen.hs:524-529, :561-566): genFilterR over
// each emitted record's aggregate object. Here that is one pass at the end of
// a push over the segment [base, base + rows) of the op's changelog columns:
// the op's postfix program (include/hstream_gpu.h hsg_where_ins, interpreted
// by hsg_pred.h) runs per row over the aggregate
// columns it names, and the rows it keeps are compacted, in order, towards
// `base` -- every column: key, window start / end, src_index, each aggregate
// and the literal forms where kept.
//
// In place, one launch, a chained scan with look-back (hsg_lookback.h) over
// tiles of kHavingTile rows (one row per thread). A workgroup takes a tile ticket (tiles
// are handed out in order, so a tile only ever waits for tiles already taken),
// reads the named columns, evaluates, ranks its kept rows (wave ballots, a
// scan of the wave counts in LDS), loads the other columns of the kept rows
// only and parks the whole kept rows in LDS at their ranks. Then it publishes
// its count, looks back for the sum of its predecessors' counts, publishes its
// inclusive sum, and writes its rows from LDS, coalesced, to base + sum.
//
// The in-place hazard: a row's destination is never above its source, so a
// tile writes onto rows of the tiles before it (and of itself). It is safe
// because a tile publishes only after all its rows are in LDS -- the loads are
// consumed by the LDS stores ahead of the workgroup barrier that precedes the
// publication -- and writes only after its look-back found every predecessor
// published (an inclusive sum stands for its publisher's predecessors too).
// No tile reads a row another tile wrote in this launch, so the row loads need
// no acquire; a tile's state is one 8-byte word (status and count together)
// moved by relaxed agent-scope atomics, so there is no payload to order
// behind a flag.
//
// Byte model, per row of the segment with c named columns, a aggregates and
// f = 4 if the op keeps literal forms else 0:
//   read    8 c                      every row (the named aggregate words)
//   read    28 + f + 8 (a - c)       kept rows only (key, ws, we, src, the rest)
//   written 28 + f + 8 a             kept rows only
// plus 8 B of tile state per 256 rows each way and one ticket atomic per tile.
// Flags: none are stored (a row's keep bit lives in a ballot). LDS: 256 whole
// rows of 160 B per workgroup, which is what bounds the resident round of
// classes 0 and 1 (hsg_where.h kGroupsPerCU; the compiler's report: DESIGN.md 5).
#include "hsg_lookback.h"
#include "hsg_pred.h"

namespace hsg {

namespace {

constexpr int T = kHavingTile;
using namespace lookback;

}  // namespace

// FC: the function class of the program (hsg_pred.h), one kernel each
template <int FC>
__global__ __launch_bounds__(T) void k_having(const WhereProg p, const HavingArgs a) {
  __shared__ uint64_t s_w[3 + kMaxAggs][T];  // ws, we, src, aggregates
  __shared__ uint32_t s_key[T], s_form[T];
  __shared__ TileLds<T / 64> s_lds;

  uint64_t total = a.host_total;
  if (total == UINT64_MAX) total = *a.tot_a + (a.tot_b ? *a.tot_b : 0);
  if (total > a.max_rows) {
    // the tile states cover max_rows, and the room check holds the rows below it
    total = a.max_rows;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&a.sc->err, ERR_HAVING);
  }
  // the host's own condition for running the emit chain it had not launched
  // (push_time_atomic, after this fetch): the batch filled the touched list
  // and had no error; the chain appends at the unfiltered count of the rows
  // the apply wrote (scratch[3]), and the pass ahead of the next fetch filters
  // all of them (uniform: the batch's kernels have finished, and the bit this
  // kernel sets is left out)
  const uint64_t how = a.sc->scratch[2];
  const bool emit_follows = a.hold_emit && how != 1 && how != 3 && (a.sc->scratch[1] | a.sc->scratch[6]) != 0 &&
                            (a.sc->err & (ERR_OOM | ERR_RANGE)) == 0;
  if (*a.skip || a.sc->redo || emit_follows || total == 0) {
    // nothing to filter, or rows the batch's next run writes again or appends to
    if (blockIdx.x == 0 && threadIdx.x == 0) a.sc->scratch[kHavingWord] = total == 0 ? kHavingRan : 0;
    return;
  }
  const uint64_t n_tiles = (total + T - 1) / T;
  const int tid = threadIdx.x;

  while (true) {
    const uint64_t t = take_tile(s_lds, a.state);
    if (t >= n_tiles) return;
    const uint64_t row = t * T + tid;
    const bool in = row < total;
    const uint64_t src = a.base + row;

    // the named aggregate words, all loads in flight before the program runs
    uint64_t cv[kMaxAggs];
#pragma unroll
    for (int c = 0; c < kMaxAggs; ++c) cv[c] = (in && ((p.cols >> c) & 1u)) ? (uint64_t)a.out.agg[c][src] : 0;
    // an f64 output that is NaN (AVG of no value) is the error value
    const bool keep = in && pred::eval<FC>(p, cv, pred::nan_mask(cv, p.cols & p.f64));
    const Rank k = rank_kept(s_lds, keep);
    const uint32_t r = k.rank, count = k.count;

    // the kept rows, whole, into LDS at their ranks: every load of the other
    // columns in flight first, then the LDS stores
    if (keep) {
      const uint32_t k = a.out.key[src];
      const int64_t ws = a.out.ws[src], we = a.out.we[src], si = a.out.src[src];
      const uint32_t fm = a.out.form ? a.out.form[src] : 0;
#pragma unroll
      for (int c = 0; c < kMaxAggs; ++c)
        if (c < a.n_aggs && !((p.cols >> c) & 1u)) cv[c] = (uint64_t)a.out.agg[c][src];
      s_key[r] = k;
      s_w[0][r] = (uint64_t)ws;
      s_w[1][r] = (uint64_t)we;
      s_w[2][r] = (uint64_t)si;
#pragma unroll
      for (int c = 0; c < kMaxAggs; ++c)
        if (c < a.n_aggs) s_w[3 + c][r] = cv[c];
      if (a.out.form) s_form[r] = fm;
    }
    // every load of the tile's rows has landed (the LDS stores consumed them)
    __syncthreads();

    const uint64_t excl = publish_tile(s_lds, a.state + 2, t, n_tiles, count, a.sc, ERR_HAVING,
                                       &a.sc->scratch[kHavingWord], kHavingRan);
    if (excl == kNoSum) return;  // uniform

    // every predecessor has its rows in LDS or written: write ours
    if ((uint32_t)tid < count) {
      const uint64_t dst = a.base + excl + tid;
      a.out.key[dst] = s_key[tid];
      a.out.ws[dst] = (int64_t)s_w[0][tid];
      a.out.we[dst] = (int64_t)s_w[1][tid];
      a.out.src[dst] = (int64_t)s_w[2][tid];
#pragma unroll
      for (int c = 0; c < kMaxAggs; ++c)
        if (c < a.n_aggs) a.out.agg[c][dst] = (int64_t)s_w[3 + c][tid];
      if (a.out.form) a.out.form[dst] = s_form[tid];
    }
    __syncthreads();  // the rows' LDS and s_lds are reused by the next tile
  }
}

void launch_having(hipStream_t s, const WhereProg &p, const HavingArgs &a, int fn_class) {
  if (!p.n || !a.max_rows) return;
  // a workgroup per tile of the host's bound; the workgroups take tiles until
  // none is left, so the grid bounds nothing but the parallelism
  launch_by_class(kPassHaving, fn_class, (a.max_rows + T - 1) / T, [&](auto fc, dim3 grid) {
    hipLaunchKernelGGL(k_having<decltype(fc)::value>, grid, dim3(T), 0, s, p, a);
  });
}

}  // namespace hsg

extern "C" int hsg_having_tile_rows(void) { return hsg::kHavingTile; }
