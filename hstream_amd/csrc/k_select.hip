// Scalar SELECT: WHERE, the SELECT list and HAVING of a query without GROUP
// BY, over each record of a staged batch.
//
// The reference compiles such a query to a chain of three stateless nodes
// (the RGroupByEmpty branch of genStreamBuilderWithStream, hstream-sql/src/
// HStream/SQL/Codegen.hs:542-550): genFilterNode whr, genMapNode sel and
// genFilteRNodeFromHaving hav, one record at a time. Here that is one launch
// per batch. The op's three programs (include/hstream_gpu.h hsg_where_ins,
// interpreted by hsg_pred.h) run per record in registers, and the records all
// three keep become changelog rows, compacted in arrival order behind the rows
// already pending: key, win_start = win_end = the record's ts, src_index, one
// 8-byte word per expression and the literal forms where kept.
//
// One launch, a chained scan with look-back (hsg_lookback.h) over tiles of
// kSelectTile records, one record per thread. A
// workgroup takes a tile ticket (tiles are handed out in order, so a tile only
// ever waits for tiles already taken), loads the key, the ts and the columns
// and valid bytes the programs name -- each once, every load in flight before
// the first instruction -- evaluates WHERE, the expressions and HAVING, ranks
// its kept records (wave ballots, a scan of the wave counts in LDS), publishes
// its count, looks back for the sum of its predecessors' counts, publishes its
// inclusive sum and writes its rows from registers to base + sum + rank. The
// last tile leaves the batch's total beside the scalars the push fetches
// anyway, so a push waits for no read of its own.
//
// Not in place: the batch is read, the changelog written, and no tile reads
// what another wrote, so there is no hazard to order and no row staging in
// LDS. The kept lanes of a wave write consecutive rows, so a column's stores
// of one wave fall in at most 64 * 8 B = four 128-byte lines plus one for the
// misalignment of base + sum: staging would save at most that one line.
//
// Byte model, per batch of N records of which K are kept, with c named
// columns of which v have a valid array, e expressions, k = 4 if the batch
// has keys else 0 and f = 4 if the op keeps literal forms else 0:
//   read    N * (k + 8 + 8 c + v)        key, ts, the named words and bytes
//   written K * (k' + 24 + 8 e + f)      key (k' = 4, always), ws, we, src,
//                                        the expressions, the form word
// plus 8 B of tile state per 256 records each way, one ticket atomic per tile
// and at most five atomics per wave at its end (the three drop counts, the
// maximum ts, which is stream time's input).
//
// A workgroup is 256 threads, one wave on each SIMD, so waves per SIMD is also
// workgroups per CU; the kernel's LDS is the protocol's few words, and its
// registers set the resident round the grid is capped to (hsg_where.h
// kGroupsPerCU; the compiler's report and the measured rates: DESIGN.md 5).
// The kernel is bound by the interpreter's instructions and the per-tile
// chain, not by HBM.
#include "hsg_lookback.h"
#include "hsg_pred.h"
#include "hsg_select.h"

namespace hsg {

namespace {

constexpr int T = kSelectTile;
using namespace lookback;

}  // namespace

// FC: the function class of the op's programs (hsg_pred.h), one kernel each
template <int FC>
__global__ __launch_bounds__(T) void k_select(const SelectProg p, const SelectArgs a) {
  __shared__ TileLds<T / 64> s_lds;

  const uint64_t n_tiles = (a.n + T - 1) / T;
  const int tid = threadIdx.x, lane = tid & 63;
  // per thread, folded per wave at the end
  uint64_t c_where = 0, c_expr = 0, c_having = 0, ts_top = 0;

  while (true) {
    const uint64_t t = take_tile(s_lds, a.state);
    if (t >= n_tiles) break;
    const uint64_t i = t * T + tid;
    const bool in = i < a.n;

    // key, ts and the named columns, all loads in flight before the programs run
    const uint32_t key = (in && a.key) ? a.key[i] : HSG_KEY_NONE;
    const int64_t ts = in ? a.ts[i] : 0;
    uint64_t cv[kMaxCols];
    uint32_t absent, cform;
    pred::load_cols(p.m.cols, a.col, a.valid, i, in, p.m.forms, cv, absent, cform);
    // stream time takes every record, skipped ones too (Processor.hs:139)
    if (in) {
      const uint64_t u = (uint64_t)ts ^ (1ull << 63);
      ts_top = u > ts_top ? u : ts_top;
    }
    const bool live = in && (!a.key || key != HSG_KEY_NONE);

    const bool w_keep = p.m.where.n ? pred::eval<FC>(p.m.where, cv, absent) : true;
    // the expressions: ev[j], bit j of e_err (the error value) and of e_form
    // (the derived literal-form bit)
    uint64_t ev[HSG_MAP_MAX_EXPRS];
#pragma unroll
    for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j) ev[j] = 0;
    uint32_t e_err = 0, e_form = 0;
    pred::run_exprs<FC>(p.m, cv, absent, cform, [&](int r, uint64_t v, uint32_t e, uint32_t form) {
#pragma unroll
      for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j) ev[j] = r == j ? v : ev[j];
      e_err |= e << r;
      e_form |= form << r;
    });
    // HAVING over the expressions: an f64 value that is NaN is the error value
    const uint32_t h_abs = e_err | pred::nan_mask(ev, p.having.cols & p.ef64);
    const bool h_keep = p.having.n ? pred::eval<FC>(p.having, ev, h_abs) : true;

    const bool keep = live && w_keep && e_err == 0 && h_keep;
    c_where += live && !w_keep ? 1 : 0;
    c_expr += live && w_keep && e_err != 0 ? 1 : 0;
    c_having += live && w_keep && e_err == 0 && !h_keep ? 1 : 0;

    // nothing is read back in place, so nothing waits between rank and publish
    const Rank k = rank_kept(s_lds, keep);
    const uint64_t excl = publish_tile(s_lds, a.state + 2, t, n_tiles, k.count, a.sc, ERR_SELECT,
                                       &a.sc->scratch[kSelectWord], kSelectRan);
    if (excl == kNoSum) break;  // uniform

    // the host's room check holds base + n <= the columns' capacity
    if (keep) {
      const uint64_t dst = a.base + excl + k.rank;
      a.out.key[dst] = key;
      a.out.ws[dst] = ts;
      a.out.we[dst] = ts;
      a.out.src[dst] = (int64_t)(a.rec_base + i);
#pragma unroll
      for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j)
        if (j < p.n_exprs) a.out.agg[j][dst] = (int64_t)ev[j];
      if (a.out.form) {
        // bit 2j: expression j prints as an integer (its derived bit 1 is clear); bit 2j + 1 stays 0
        uint32_t fm = 0;
#pragma unroll
        for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j)
          if (j < p.n_exprs) fm |= (((e_form >> j) & 1u) ^ 1u) << (2 * j);
        a.out.form[dst] = fm;
      }
    }
    __syncthreads();  // s_lds is reused by the next tile
  }

  // at most one atomic per wave and word
  const uint64_t nw = wave_sum(c_where), ne = wave_sum(c_expr), nh = wave_sum(c_having), top = wave_max(ts_top);
  if (lane == 0) {
    if (nw) atomicAdd((unsigned long long *)&a.sc->scratch[kSelWhereWord], (unsigned long long)nw);
    if (ne) atomicAdd((unsigned long long *)&a.sc->scratch[kSelExprWord], (unsigned long long)ne);
    if (nh) atomicAdd((unsigned long long *)&a.sc->scratch[kSelHavingWord], (unsigned long long)nh);
    if (top) atomicMax((unsigned long long *)&a.sc->scratch[kSelTsWord], (unsigned long long)top);
  }
}

void launch_select(hipStream_t s, const SelectProg &p, const SelectArgs &a, int fn_class) {
  if (!a.n) return;
  // a workgroup per tile; the workgroups take tiles until none is left, so the
  // grid bounds nothing but the parallelism
  launch_by_class(kPassSelect, fn_class, (a.n + T - 1) / T, [&](auto fc, dim3 grid) {
    hipLaunchKernelGGL(k_select<decltype(fc)::value>, grid, dim3(T), 0, s, p, a);
  });
}

}  // namespace hsg

extern "C" int hsg_select_tile_rows(void) { return hsg::kSelectTile; }
extern "C" int hsg_select_grid_groups(void) { return hsg::pass_grid(hsg::kPassSelect, 0); }
