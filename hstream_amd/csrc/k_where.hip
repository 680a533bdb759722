// WHERE pushdown: the SQL filter over a staged batch, ahead of the aggregate.
//
// The reference runs genFilterR (hstream-sql/src/HStream/SQL/Codegen.hs:303-341)
// as a node of its own in front of the aggregate, one record at a time; a
// record it drops, or one whose getFieldByName throws (Internal/Codegen.hs:
// 41-49), has already moved the task's stream time (Processor.hs:139-143).
// Here that is "the key becomes HSG_KEY_NONE": one pass over the staged batch
// interprets the op's postfix program (include/hstream_gpu.h hsg_where_ins)
// per record and stores the key or HSG_KEY_NONE; nothing is compacted, so
// src_index, stream time and every later kernel see the batch they always saw.
//
// Per record the pass moves the key in and out (4 + 4 B) and, of the columns
// the program names only, the value and the valid byte (9 B):
//   bytes = N * (8 + 9 * named columns).
// The program arrives as a kernel argument and is interpreted by hsg_pred.h:
// scalar opcodes, a register stack, a per-lane error bit beside each entry.
// The grid is one resident round (hsg_where.h kGroupsPerCU; the compiler's
// report: DESIGN.md 5).
#include "hsg_pred.h"

namespace hsg {

constexpr int kWhereThreads = 256;

// FC: the function class of the program (hsg_pred.h), one kernel each
template <int FC>
__global__ __launch_bounds__(kWhereThreads) void k_where(const WhereProg p, const WhereArgs a) {
  const uint64_t stride = (uint64_t)gridDim.x * kWhereThreads;
  uint64_t dropped = 0;
  // whole waves iterate together (the bound is rounded up to the wave), so the
  // ballot below sees every lane of the wave
  const uint64_t n_up = (a.n + 63) & ~63ull;
  for (uint64_t i = blockIdx.x * (uint64_t)kWhereThreads + threadIdx.x; i < n_up; i += stride) {
    const bool in = i < a.n;
    const uint32_t key = in ? a.key[i] : HSG_KEY_NONE;
    // the named columns; a predicate reads no literal form
    uint64_t cv[kMaxCols];
    uint32_t absent, cform;
    pred::load_cols(p.cols, a.col, a.valid, i, in, 0u, cv, absent, cform);
    const bool keep = pred::eval<FC>(p, cv, absent);
    const bool drop = key != HSG_KEY_NONE && !keep;
    if (in) a.out[i] = drop ? HSG_KEY_NONE : key;
    const uint64_t m = __ballot(drop);
    if ((threadIdx.x & 63) == 0) dropped += (uint64_t)__popcll(m);
  }
  // one atomic per wave
  if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(a.dropped, (unsigned long long)dropped);
}

void launch_where(hipStream_t s, const WhereProg &p, const WhereArgs &a, int fn_class) {
  if (!a.n || !p.n) return;
  // a larger batch strides
  launch_by_class(kPassWhere, fn_class, (a.n + kWhereThreads - 1) / kWhereThreads, [&](auto fc, dim3 grid) {
    hipLaunchKernelGGL(k_where<decltype(fc)::value>, grid, dim3(kWhereThreads), 0, s, p, a);
  });
}

}  // namespace hsg
