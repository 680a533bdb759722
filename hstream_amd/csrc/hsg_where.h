// The row programs of include/hstream_gpu.h (hsg_where_ins) as the host checks
// and compiles them (hsg_api.cpp) and as the passes take them: the WHERE
// filter, the computed columns and the HAVING filter, with how each pass is
// launched (the interpreter itself: hsg_pred.h). Not part of the ABI.
#pragma once

#include <string>
#include <type_traits>

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
  uint32_t fn_class;                   // host only: the kernel the program runs on (prog_fn_class)
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

// The function class of a program (hsg_prog_fn_class): 0 no HSG_W_FN, 1 the
// exact family only (ABS, CEIL, FLOOR, ROUND, SIGN, SQRT), 2 any other.
int prog_fn_class(const hsg_where_ins *prog, int32_t n);

// ---- launching a pass ----------------------------------------------------------
// Every pass that interprets a program is one kernel template over the
// function class (hsg_pred.h), launched as one resident round of workgroups: a
// grid past what is resident runs a second, mostly empty round, and a smaller
// one also keeps the per-wave atomics few. Workgroups of 256 threads per CU,
// by pass and function class, from the kernels' reported occupancy (the table
// of DESIGN.md 5): k_where fits 7 in classes 0 and 1 and takes 6; k_having's
// classes 0 and 1 are bound by LDS, every other entry by registers.
enum Pass { kPassWhere, kPassMap, kPassHaving, kPassSelect };
constexpr int kCUs = 256;
constexpr int kGroupsPerCU[4][3] = {
    /* k_where  */ {6, 6, 2},
    /* k_map    */ {7, 7, 2},
    /* k_having */ {3, 3, 2},
    /* k_select */ {4, 4, 2},
};
constexpr int pass_grid(Pass pass, int fn_class) { return kCUs * kGroupsPerCU[pass][fn_class]; }

// launch(fc, grid) with fc an integral constant of fn_class, so the caller
// names its kernel template once: k<decltype(fc)::value>. grid is `groups`
// (the workgroups the work would fill) capped to the pass's resident round.
template <class F>
inline void launch_by_class(Pass pass, int fn_class, uint64_t groups, F &&launch) {
  const uint64_t cap = (uint64_t)pass_grid(pass, fn_class);
  const dim3 grid((unsigned)(groups < cap ? groups : cap));
  if (fn_class == 0) launch(std::integral_constant<int, 0>(), grid);
  else if (fn_class == 1) launch(std::integral_constant<int, 1>(), grid);
  else launch(std::integral_constant<int, 2>(), grid);
}

void launch_where(hipStream_t s, const WhereProg &p, const WhereArgs &a, int fn_class);

// ---- computed columns (k_map.hip) ---------------------------------------------
// The op's map (include/hstream_gpu.h hsg_map_expr) as the pass runs it: the
// value programs of the expressions the pass has work for, concatenated. An
// expression that is a single COL is an alias (MapPlan::alias) and is
// here only when it is strict, for its error bit. The op's WHERE program, if
// any, travels in the same argument and runs first.
constexpr int kMapThreads = 256;

struct MapProg {
  WhereProg where;                     // where.n == 0: no filter
  int32_t n_ins;                       // instructions of all runs together
  int32_t n_runs;                      // expressions evaluated
  uint32_t cols;                       // bit c: WHERE or an expression names column c
  uint32_t forms;                      // 1: HSG_OPF_LITERAL_FORMS, the derived valid bytes carry bit 1
  int32_t end[HSG_MAP_MAX_EXPRS];      // run r is ins[end[r-1] .. end[r])
  int32_t out[HSG_MAP_MAX_EXPRS];      // the output it stores (MapArgs::ocol), -1: none (a strict alias)
  uint32_t strict;                     // bit r: run r is HSG_MAP_STRICT
  uint32_t f64;                        // bit c: column c is HSG_F64
  // (I64 / F64 constants carry their literal-form bit in `arg`)
  hsg_where_ins ins[HSG_MAP_MAX_INS];
};

struct MapArgs {
  uint64_t n;
  const uint32_t *key;                 // staged keys
  uint32_t *out;                       // masked keys (op-owned; may be `key`), null: the keys stay as they are
  const int64_t *col[kMaxCols];        // the batch's columns (the caller's numbering)
  const uint8_t *valid[kMaxCols];      // null = all present
  int64_t *ocol[HSG_MAP_MAX_EXPRS];    // computed outputs (op-owned staging)
  uint8_t *ovalid[HSG_MAP_MAX_EXPRS];  // null: every byte would be 1, none is written
  // two cumulative 32-bit counts: [0] += keyed records WHERE masked, [1] +=
  // keyed records WHERE kept and a strict expression dropped
  unsigned int *dropped;
};

// What the host keeps of the map beside the kernel's program.
struct MapPlan {
  int32_t n_exprs = 0;                    // 0: the op has no map
  int32_t n_out = 0;                      // computed outputs
  int32_t alias[HSG_MAP_MAX_EXPRS] = {};  // expression j is the caller's column alias[j]; -1: computed
  int32_t ocol[HSG_MAP_MAX_EXPRS] = {};   // ... or output ocol[j] of the pass
  uint32_t reads[HSG_MAP_MAX_EXPRS] = {}; // the columns expression j names
  bool const_form[HSG_MAP_MAX_EXPRS] = {};// expression j holds a constant whose literal-form bit is 1
  // expression j holds a function that can give the error value or a literal-
  // form bit of its own: any but ABS / CEIL / FLOOR / ROUND / SIGN of an i64
  bool fn_valid[HSG_MAP_MAX_EXPRS] = {};
  bool keys = false;                      // the pass writes keys (a WHERE program or a strict expression)
  int32_t fn_class = 0;                   // the kernel the pass runs: the maximum over WHERE and the expressions
};

// Type-check a map (hsg_map_check): HSG_OK with out_types (may be null), or HSG_E_INVALID with err set.
int map_check(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols, int32_t *out_types,
              std::string &err);
// (checked map; `where` compiled or n == 0) -> MapProg + MapPlan
void map_compile(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols, bool forms,
                 const WhereProg &where, MapProg &out, MapPlan &plan);
void launch_map(hipStream_t s, const MapProg &p, const MapArgs &a, int fn_class);

// ---- HAVING pushdown (k_having.hip) ------------------------------------------
// The same program over an op's changelog rows: column c is aggregate c of the
// op (WhereProg::cols / f64 are 32-bit masks, kMaxAggs is 16).

// Rows of one compaction tile (hsg_having_tile_rows).
constexpr int kHavingTile = 256;

// DevScalars::scratch word of the pass: bit 63 = the pass ran over the batch's
// rows, the low bits = the rows it kept. A per-batch word (the clears zero
// it): a batch whose kernels run more than once is filtered ahead of every
// fetch of its scalars, and only the last fetch -- the batch's final rows --
// is the one the host reads the word from (hsg_api.cpp push_sync). A fetch the
// host will follow with another run of the batch (held back for table room,
// late records under the optimistic path) finds the pass idle: k_having skips
// when HavingArgs::skip or DevScalars::redo is set, so no row is filtered
// twice, and the dropped-row count is taken from one pass. The same holds for
// a fetch the host follows with the emit chain it had not launched
// (HavingArgs::hold_emit, push_time_atomic): that chain appends behind the
// rows the apply wrote, at their unfiltered count, so those rows stay where
// they are until the chain has run.
constexpr int kHavingWord = 7;
constexpr uint64_t kHavingRan = 1ull << 63;
// DevScalars::err bit: a tile waited past its bound for its predecessors
constexpr uint32_t ERR_HAVING = 4u;

struct HavingArgs {
  OutCols out;             // the changelog columns (the op's own or the registered ones)
  uint64_t base;           // first row of the batch's segment (the pending rows before it)
  uint64_t max_rows;       // the host's bound on the segment (the tile states cover it)
  int32_t n_aggs;
  // the host did not launch the per-batch emit chain (it predicted a batch whose
  // changelog the apply writes itself): when the batch filled the touched list
  // after all, the host runs the chain after this fetch and fetches again, and
  // the pass ahead of that fetch filters the whole segment
  int32_t hold_emit;
  // the segment's length: host_total unless it is UINT64_MAX, then
  // *tot_a + *tot_b (tot_b may be null) as the batch's kernels left them
  uint64_t host_total;
  const uint64_t *tot_a, *tot_b;
  const uint64_t *skip;    // non-zero: the batch will run again, leave the rows alone
  uint64_t *state;         // [0] tile tickets, [2 ..] one word per tile; zeroed before the launch
  DevScalars *sc;
};

// Type-check a HAVING program against the op's aggregate outputs (hsg_having_check).
int having_check(const hsg_where_ins *prog, int32_t n, const hsg_op_config *cfg, std::string &err);
// the value type of each aggregate output: COUNT_ALL / COUNT i64, AVG f64, else the column's
void having_types(const hsg_op_config *cfg, int32_t *types);

// words of an ordered compaction's state (HavingArgs::state, SelectArgs::state)
// for up to `rows` rows in tiles of `tile`: the ticket, a pad, one per tile
inline uint64_t tile_state_words(uint64_t rows, int tile) { return ((rows / tile + 1 + 2) + 1) & ~1ull; }
void launch_having(hipStream_t s, const WhereProg &p, const HavingArgs &a, int fn_class);

}  // namespace hsg
