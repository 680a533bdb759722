// Scalar SELECT (k_select.hip): the op without a group key -- WHERE, the SELECT
// list's value programs and HAVING over each record of a staged batch, the
// kept rows compacted in arrival order into the changelog columns
// (include/hstream_gpu.h "Scalar SELECT"). Not part of the ABI.
#pragma once

#include <string>

#include "hsg_where.h"

namespace hsg {

// Records of one tile (hsg_select_tile_rows): one record per thread.
constexpr int kSelectTile = 256;

// DevScalars::scratch words of the pass, per batch (the clears zero them; no
// other kernel runs on a select op's scalars):
constexpr int kSelectWord = 7;     // bit 63 = the pass ran to its last tile, low bits = rows kept
constexpr int kSelWhereWord = 8;   // live records WHERE dropped
constexpr int kSelExprWord = 9;    // ... WHERE kept and an expression's error value dropped
constexpr int kSelHavingWord = 10; // ... both kept and HAVING dropped
constexpr int kSelTsWord = 11;     // max ts of the batch + 2^63 as a u64 (0: no record)
constexpr uint64_t kSelectRan = 1ull << 63;
// DevScalars::err bit: a tile waited past its bound for its predecessors
constexpr uint32_t ERR_SELECT = 8u;

// The op's three programs as the kernel takes them (one kernel argument).
// m.where is the WHERE program (n == 0: none); m.ins / m.end are the value
// programs, run r = expression r (every one strict, aliases included);
// having names the expressions (n == 0: none), ef64 bit j: expression j is f64.
struct SelectProg {
  MapProg m;
  WhereProg having;
  int32_t n_exprs;
  uint32_t ef64;
};

struct SelectArgs {
  uint64_t n;
  const uint32_t *key;             // null: every record is live and its row carries HSG_KEY_NONE
  const int64_t *ts;
  const int64_t *col[kMaxCols];    // the batch's columns (the caller's numbering)
  const uint8_t *valid[kMaxCols];  // null = all present
  OutCols out;                     // the changelog columns (the op's own or the registered ones)
  uint64_t base;                   // rows pending ahead of the batch: the first row it may write
  uint64_t rec_base;               // global index of record 0 (src_index)
  uint64_t *state;                 // [0] tile tickets, [2 ..] one word per tile; zeroed before the launch
  DevScalars *sc;
};
static_assert(sizeof(SelectProg) + sizeof(SelectArgs) <= 4096, "kernel arguments");

// Type-check the three programs (hsg_select_check): HSG_OK with the
// expressions' static types in out_types (may be null), or HSG_E_INVALID with
// err set ("where: ", "select: " / "map: expr j: ", "having: ").
int select_check(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                 const hsg_where_ins *having, int32_t n_having, const int32_t *col_types, int32_t n_cols,
                 int32_t *out_types, std::string &err);
// (checked programs, expr_types as select_check left them) -> SelectProg;
// returns the kernel's function class
int select_compile(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                   const hsg_where_ins *having, int32_t n_having, const int32_t *col_types, int32_t n_cols,
                   const int32_t *expr_types, bool forms, SelectProg &out);
void launch_select(hipStream_t s, const SelectProg &p, const SelectArgs &a, int fn_class);

}  // namespace hsg
