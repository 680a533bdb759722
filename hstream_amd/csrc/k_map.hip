// Computed columns: the SELECT list's value expressions over a staged batch,
// ahead of the aggregate (include/hstream_gpu.h hsg_map_expr).
//
// The reference evaluates genRExprValue per record inside the aggregate
// (genAggregateComponentsFromDerivedCol, hstream-sql/src/HStream/SQL/
// Codegen.hs:463-469). Here one pass over the staged batch interprets the
// op's value programs per record and stores one 8-byte word per computed
// expression, with its valid byte where one is needed, into op-owned staging;
// the aggregation kernels then read those as the columns they always read.
// An op with a WHERE program runs it here too, ahead of the expressions, so
// each named column is read once: the verdict first (hsg_pred.h eval), then
// every expression. A record the filter drops, or one whose strict expression
// is the error value, leaves with HSG_KEY_NONE; nothing is compacted.
//
// Per record the pass moves the key in and out when it writes keys (4 + 4 B),
// of the named columns the value and the valid byte (9 B), and per computed
// output the value and, where written, its valid byte:
//   bytes = N * (8 * [keys written] + 9 * named columns
//                + (8 + [valid written]) * computed outputs).
// The programs arrive as one kernel argument and are interpreted by
// hsg_pred.h run_exprs: scalar opcodes, a register stack, a per-lane error bit
// and literal-form bit beside each entry. The grid is one resident round
// (hsg_where.h kGroupsPerCU; the compiler's report: DESIGN.md 5).
#include "hsg_pred.h"

namespace hsg {

// FC: the function class of the op's programs (hsg_pred.h), one kernel each
template <int FC>
__global__ __launch_bounds__(kMapThreads) void k_map(const MapProg p, const MapArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kMapThreads;
  uint64_t w_dropped = 0, m_dropped = 0;
  // whole waves iterate together (the bound is rounded up to the wave), so the
  // ballots below see every lane of the wave
  const uint64_t n_up = (a.n + 63) & ~63ull;
  for (uint64_t i = blockIdx.x * (uint64_t)kMapThreads + threadIdx.x; i < n_up; i += stride) {
    const bool in = i < a.n;
    const uint32_t key = in ? a.key[i] : HSG_KEY_NONE;
    uint64_t cv[kMaxCols];
    uint32_t absent, cform;
    pred::load_cols(p.cols, a.col, a.valid, i, in, p.forms, cv, absent, cform);
    const bool keep = p.where.n ? pred::eval<FC>(p.where, cv, absent) : true;
    bool strict_err = false;
    pred::run_exprs<FC>(p, cv, absent, cform, [&](int r, uint64_t v, uint32_t e, uint32_t form) {
      strict_err |= e && ((p.strict >> r) & 1u);
      const int o = p.out[r];
      if (o >= 0 && in) {
        a.ocol[o][i] = (int64_t)v;
        // (absent is the whole byte 0: the aggregates take any other byte as present)
        if (a.ovalid[o]) a.ovalid[o][i] = e ? (uint8_t)0 : (uint8_t)(1u | ((form & p.forms) << 1));
      }
    });
    const bool keyed = key != HSG_KEY_NONE;
    const bool w_drop = keyed && !keep;
    const bool m_drop = keyed && keep && strict_err;
    if (in && a.out) a.out[i] = (w_drop || m_drop) ? HSG_KEY_NONE : key;
    const uint64_t mw = __ballot(w_drop), mm = __ballot(m_drop);
    if ((threadIdx.x & 63) == 0) {
      w_dropped += (uint64_t)__popcll(mw);
      m_dropped += (uint64_t)__popcll(mm);
    }
  }
  // at most one atomic per wave and count
  if ((threadIdx.x & 63) == 0) {
    if (w_dropped) atomicAdd(&a.dropped[0], (unsigned int)w_dropped);
    if (m_dropped) atomicAdd(&a.dropped[1], (unsigned int)m_dropped);
  }
}

void launch_map(hipStream_t s, const MapProg &p, const MapArgs &a, int fn_class) {
  if (!a.n || (!p.n_ins && !p.where.n)) return;
  // a larger batch strides
  launch_by_class(kPassMap, fn_class, (a.n + kMapThreads - 1) / kMapThreads, [&](auto fc, dim3 grid) {
    hipLaunchKernelGGL(k_map<decltype(fc)::value>, grid, dim3(kMapThreads), 0, s, p, a);
  });
}

}  // namespace hsg
