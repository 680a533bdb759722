// WHERE pushdown: the predicate program of include/hstream_gpu.h
// (hsg_where_ins) as the host checks it (hsg_api.cpp where_check) and as
// k_where.hip interprets it over a staged batch. Not part of the ABI.
#pragma once

#include <string>

#include "hsg_internal.h"

namespace hsg {

// DevScalars::scratch word of the records k_where masked: cumulative since
// create / reset -- the per-batch clears (k_clear_scalars,
// k_fetch_clear_scalars) leave it alone, so a batch that runs its kernels
// twice (replays) still reports the one filter pass it had; the host takes
// the difference between two fetches (hsg_stats.where_dropped).
constexpr int kWhereWord = 35;

// One op's program, passed to the kernel by value (kernel arguments: the
// instruction stream is read with scalar loads, uniform over the wave).
struct WhereProg {
  int32_t n;                           // 0 = the op has no WHERE
  uint32_t cols;                       // bit c: the program names column c
  uint32_t f64;                        // bit c: column c is HSG_F64
  uint32_t reserved;
  hsg_where_ins ins[HSG_WHERE_MAX_INS];
};

struct WhereArgs {
  uint64_t n;
  const uint32_t *key;                 // staged keys
  uint32_t *out;                       // masked keys (op-owned; may be `key`)
  const int64_t *col[kMaxCols];        // the batch's columns (the caller's numbering)
  const uint8_t *valid[kMaxCols];      // null = all present
  unsigned long long *dropped;         // += keyed records the program masked
};

// Type-check a program (hsg_where_check): HSG_OK, or HSG_E_INVALID with err set.
int where_check(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, std::string &err);
// (checked program) -> WhereProg
void where_compile(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, WhereProg &out);

void launch_where(hipStream_t s, const WhereProg &p, const WhereArgs &a);

}  // namespace hsg
