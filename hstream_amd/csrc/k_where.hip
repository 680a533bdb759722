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
// The program arrives as a kernel argument and is interpreted by hsg_pred.h
// (shared with the HAVING pass, k_having.hip): scalar opcodes, a register
// stack, a per-lane error bit beside each entry.
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
    // the named columns, all loads in flight before the program runs
    uint64_t cv[kMaxCols];
    uint32_t absent = 0;
#pragma unroll
    for (int c = 0; c < kMaxCols; ++c) {
      cv[c] = 0;
      if ((p.cols >> c) & 1u) {
        if (in) cv[c] = (uint64_t)a.col[c][i];
        // bit 0 alone says present; bit 1 is the literal form
        if (in && a.valid[c] && !(a.valid[c][i] & 1u)) absent |= 1u << c;
      }
    }
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
  // one resident round of workgroups: 6 per CU of 256 CUs (the kernel fits 7,
  // 28 waves per CU; a grid past what is resident runs a second, mostly empty
  // round), which also keeps the per-wave atomics to a few thousand
  uint64_t g = (a.n + kWhereThreads - 1) / kWhereThreads;
  // (the function classes: a round of their own occupancy)
  const uint64_t cap = 256 * (uint64_t)(fn_class == 0 ? 6 : (fn_class == 1 ? kWhereGroupsFn1 : kWhereGroupsFn2));
  if (g > cap) g = cap;
  if (fn_class == 0) hipLaunchKernelGGL(k_where<0>, dim3((unsigned)g), dim3(kWhereThreads), 0, s, p, a);
  else if (fn_class == 1) hipLaunchKernelGGL(k_where<1>, dim3((unsigned)g), dim3(kWhereThreads), 0, s, p, a);
  else hipLaunchKernelGGL(k_where<2>, dim3((unsigned)g), dim3(kWhereThreads), 0, s, p, a);
}

}  // namespace hsg
