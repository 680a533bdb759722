// Scalar SELECT: WHERE, the SELECT list and HAVING of a query without GROUP
// BY, over each record of a staged batch.
//
// The reference compiles such a query to a chain of three stateless nodes
// (the RGroupByEmpty branch of genStreamBuilderWithStream, hstream-sql/src/
// HStream/SQL/Codegen.hs:542-550): genFilterNode whr, genMapNode sel and
// genFilteRNodeFromHaving hav, one record at a time. Here that is one launch
// per batch. The op's three programs (include/hstream_gpu.h hsg_where_ins,
// interpreted by hsg_pred.h exactly as k_where / k_map / k_having do) run per
// record in registers, and the records all three keep become changelog rows,
// compacted in arrival order behind the rows already pending: key, win_start
// = win_end = the record's ts, src_index, one 8-byte word per expression and
// the literal forms where kept.
//
// One launch, a chained scan with look-back (hsg_lookback.h, the protocol of
// k_having.hip) over tiles of kSelectTile records, one record per thread. A
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
// Budget per workgroup of 256 threads (four waves, one per SIMD). LDS: 32 B
// (the wave counts, the ticket, the offset) of the CU's 160 KiB, never the
// limit. Registers, from the compiler's report for gfx950 (512 VGPRs per SIMD
// lane allocated in eights, so waves per SIMD = 512 / allocation, at most 8;
// a workgroup is one wave on each SIMD, so that is also workgroups per CU):
//   class 0 (no function)        100 VGPRs   4 workgroups per CU
//   class 1 (the exact family)   102 VGPRs   4
//   class 2 (all 22 functions)   256 VGPRs   2
// no scratch in any. The grid is one resident round of those over 256 CUs
// (hsg_select.h kSelectGroupsFn*). Measured on an MI355X: 2^22
// records with three named columns take 0.26 - 0.31 ms with one expression and
// 0.47 - 0.51 ms with eight, 0.3 - 1.2 TB/s of the model's bytes: the kernel is
// bound by the interpreter's instructions and the per-tile chain, not by HBM.
#include "hsg_lookback.h"
#include "hsg_pred.h"
#include "hsg_select.h"

namespace hsg {

namespace {

constexpr int T = kSelectTile;
constexpr int kWaves = T / 64;
using namespace lookback;

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

}  // namespace

// FC: the function class of the op's programs (hsg_pred.h), one kernel each
template <int FC>
__global__ __launch_bounds__(T) void k_select(const SelectProg p, const SelectArgs a) {
  __shared__ uint32_t s_wcnt[kWaves];
  __shared__ uint64_t s_tile, s_excl;

  const uint64_t n_tiles = (a.n + T - 1) / T;
  uint64_t *ticket = a.state, *tiles = a.state + 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // per thread, folded per wave at the end
  uint64_t c_where = 0, c_expr = 0, c_having = 0, ts_top = 0;

  while (true) {
    if (tid == 0) s_tile = atomicAdd((unsigned long long *)ticket, 1ull);
    __syncthreads();
    const uint64_t t = s_tile;
    if (t >= n_tiles) break;
    const uint64_t i = t * T + tid;
    const bool in = i < a.n;

    // key, ts and the named columns, all loads in flight before the programs run
    const uint32_t key = (in && a.key) ? a.key[i] : HSG_KEY_NONE;
    const int64_t ts = in ? a.ts[i] : 0;
    uint64_t cv[kMaxCols];
    uint32_t vb[kMaxCols];
#pragma unroll
    for (int c = 0; c < kMaxCols; ++c) {
      cv[c] = 0;
      vb[c] = 1;
      if ((p.m.cols >> c) & 1u) {
        if (in) cv[c] = (uint64_t)a.col[c][i];
        if (in && a.valid[c]) vb[c] = a.valid[c][i];
      }
    }
    // bit 0 alone says present; bit 1 is the literal form
    uint32_t absent = 0, cform = 0;
#pragma unroll
    for (int c = 0; c < kMaxCols; ++c) {
      absent |= ((vb[c] & 1u) ^ 1u) << c;
      cform |= ((vb[c] >> 1) & 1u) << c;
    }
    if (!p.m.forms) cform = 0;
    // stream time takes every record, skipped ones too (Processor.hs:139)
    if (in) {
      const uint64_t u = (uint64_t)ts ^ (1ull << 63);
      ts_top = u > ts_top ? u : ts_top;
    }
    const bool live = in && (!a.key || key != HSG_KEY_NONE);

    const bool w_keep = p.m.where.n ? pred::eval<FC>(p.m.where, cv, absent) : true;
    // the expressions, one run after the other on one stack: ev[j], bit j of
    // e_err (the error value) and of e_form (the derived literal-form bit)
    uint64_t ev[HSG_MAP_MAX_EXPRS];
#pragma unroll
    for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j) ev[j] = 0;
    uint32_t e_err = 0, e_form = 0;
    {
      pred::Stack st;
      st.clear();
      int r = 0;
      for (int pc = 0; pc < p.m.n_ins; ++pc) {
        pred::value_step<FC>(st, p.m.ins[pc], p.m.f64, cv, absent, cform);
        if (pc + 1 == p.m.end[r]) {
          // the run's one value is the top of the stack
#pragma unroll
          for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j) ev[j] = r == j ? st.v[0] : ev[j];
          e_err |= (st.err & 1u) << r;
          e_form |= (st.form & 1u) << r;
          st.pop();
          ++r;
        }
      }
    }
    // HAVING over the expressions: an f64 value that is NaN is the error value
    uint32_t h_abs = e_err;
#pragma unroll
    for (int j = 0; j < HSG_MAP_MAX_EXPRS; ++j) {
      const double d = pred::as_f64(ev[j]);
      if (((p.having.cols & p.ef64) >> j) & 1u) h_abs |= d != d ? 1u << j : 0u;
    }
    const bool h_keep = p.having.n ? pred::eval<FC>(p.having, ev, h_abs) : true;

    const bool keep = live && w_keep && e_err == 0 && h_keep;
    c_where += live && !w_keep ? 1 : 0;
    c_expr += live && w_keep && e_err != 0 ? 1 : 0;
    c_having += live && w_keep && e_err == 0 && !h_keep ? 1 : 0;

    // rank among the tile's kept records
    const uint64_t m = __ballot(keep);
    if (lane == 0) s_wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, count = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      before += w < wave ? s_wcnt[w] : 0;
      count += s_wcnt[w];
    }
    const uint32_t r = before + (uint32_t)__popcll(m & ((1ull << lane) - 1));

    if (wave == 0) {
      if (lane == 0) st_store(tiles + t, kStAgg | count);
      const uint64_t excl = look_back(tiles, t, a.sc, ERR_SELECT);
      if (lane == 0) {
        s_excl = excl;
        if (excl != kNoSum) {
          st_store(tiles + t, kStSum | (excl + count));
          if (t == n_tiles - 1) a.sc->scratch[kSelectWord] = kSelectRan | (excl + count);
        }
      }
    }
    __syncthreads();
    const uint64_t excl = s_excl;
    if (excl == kNoSum) break;  // uniform

    // the host's room check holds base + n <= the columns' capacity
    if (keep) {
      const uint64_t dst = a.base + excl + r;
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
    __syncthreads();  // s_tile, s_excl and s_wcnt are reused by the next tile
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
  // a workgroup per tile, at most one resident round (select_grid, from the
  // kernel's registers); the workgroups take tiles until none is left, so the
  // grid bounds nothing but the parallelism
  uint64_t g = (a.n + T - 1) / T;
  const uint64_t cap = (uint64_t)select_grid(fn_class);
  if (g > cap) g = cap;
  if (fn_class == 0) hipLaunchKernelGGL(k_select<0>, dim3((unsigned)g), dim3(T), 0, s, p, a);
  else if (fn_class == 1) hipLaunchKernelGGL(k_select<1>, dim3((unsigned)g), dim3(T), 0, s, p, a);
  else hipLaunchKernelGGL(k_select<2>, dim3((unsigned)g), dim3(T), 0, s, p, a);
}

}  // namespace hsg

extern "C" int hsg_select_tile_rows(void) { return hsg::kSelectTile; }
extern "C" int hsg_select_grid_groups(void) { return hsg::select_grid(0); }
