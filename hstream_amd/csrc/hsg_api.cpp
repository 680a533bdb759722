// libhstream_gpu host runtime: the C ABI of include/hstream_gpu.h.
//
// One hsg_engine per process and GPU (device selection, RCCL communicator);
// one hsg_op per windowed GROUP BY operator. Each op owns a HIP stream, its
// HBM state (hash table of (key, window) rows, or the session arena), staging
// buffers for host batches and an HBM changelog buffer drained by hsg_drain.
// Every entry point catches everything: no C++ exception crosses the ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "hsg_internal.h"
#include "hsg_kernels.h"
#include "hsg_ops.h"
#include "hsg_where.h"

using namespace hsg;

// ---------------------------------------------------------------------------
// error helpers
// ---------------------------------------------------------------------------
#define HIP_TRY(obj, expr)                                                         \
  do {                                                                             \
    hipError_t _e = (expr);                                                        \
    if (_e != hipSuccess) {                                                        \
      (obj)->err = std::string(#expr) + ": " + hipGetErrorString(_e);              \
      return _e == hipErrorOutOfMemory ? HSG_E_OOM : HSG_E_DEVICE;                 \
    }                                                                              \
  } while (0)

namespace {

int fail(std::string &err, int code, const std::string &msg) {
  err = msg;
  return code;
}

uint64_t next_pow2(uint64_t v) {
  uint64_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

}  // namespace

// ---------------------------------------------------------------------------
// program (aggregates -> state slots -> output columns)
// ---------------------------------------------------------------------------
namespace hsg {

int build_program(const hsg_op_config &cfg, const std::vector<int32_t> &col_types, const std::vector<hsg_agg> &aggs,
                  Program &prog, std::string &err, bool forms) {
  memset(&prog, 0, sizeof(prog));
  auto find_slot = [&](int op, int col) -> int {
    for (int s = 0; s < prog.n_slots; ++s)
      if (prog.slot_op[s] == op && prog.slot_col[s] == col) return s;
    return -1;
  };
  auto add_slot = [&](int op, int col) -> int {
    int s = find_slot(op, col);
    if (s >= 0) return s;
    if (prog.n_slots >= kMaxSlots) return -1;
    prog.slot_op[prog.n_slots] = op;
    prog.slot_col[prog.n_slots] = col;
    return prog.n_slots++;
  };
  // LAST: the (record seq, value) slot pair of column c; -1 = no room
  auto last_pair = [&](int c) -> int {
    int s = find_slot(S_LAST_SEQ, c);
    if (s < 0) {
      if (prog.n_slots + 2 > kMaxSlots) return -1;
      s = add_slot(S_LAST_SEQ, c);
      prog.slot_op[prog.n_slots] = S_LAST_VAL;
      prog.slot_col[prog.n_slots] = c;
      prog.n_slots++;
    }
    return s;
  };
  if ((int)aggs.size() > kMaxAggs) return fail(err, HSG_E_INVALID, "too many aggregates (max 16)");
  for (size_t j = 0; j < aggs.size(); ++j) {
    const hsg_agg &g = aggs[j];
    int a = -1, b = 0, kind = O_I64;
    bool isf = g.kind != HSG_COUNT_ALL && col_types[g.column] == HSG_F64;
    int c = g.kind == HSG_COUNT_ALL ? 0 : g.column;
    switch (g.kind) {
      case HSG_COUNT_ALL: a = add_slot(S_CNT_ALL, 0); break;
      case HSG_COUNT: a = add_slot(S_CNT, c); break;
      case HSG_SUM: a = add_slot(isf ? S_SUM_F : S_SUM_I, c); kind = isf ? O_F64 : O_I64; break;
      case HSG_MIN: a = add_slot(isf ? S_MIN_F : S_MIN_I, c); kind = isf ? O_F64_ORD : O_I64; break;
      case HSG_MAX: a = add_slot(isf ? S_MAX_F : S_MAX_I, c); kind = isf ? O_F64_ORD : O_I64; break;
      case HSG_AVG:
        a = add_slot(isf ? S_SUM_F : S_SUM_I, c);
        b = add_slot(S_CNT, c);
        kind = isf ? O_AVG_F : O_AVG_I;
        break;
      case HSG_LAST: {
        // sessions: merges keep the existing session's value (k_session.hip)
        const int s = last_pair(c);
        if (s < 0) return fail(err, HSG_E_INVALID, "too many state slots");
        a = s + 1;
        kind = isf ? O_F64 : O_I64;
        break;
      }
      default: return fail(err, HSG_E_INVALID, "bad aggregate kind");
    }
    if (a < 0 || b < 0) return fail(err, HSG_E_INVALID, "too many state slots");
    prog.out_kind[j] = kind;
    prog.out_a[j] = a;
    prog.out_b[j] = b;
    // the literal form (hsg_internal.h FormKind): a form slot over the
    // output's column that reads bit 1 of its valid bytes
    int fk = F_NONE, fa = 0;
    if (forms) {
      switch (g.kind) {
        case HSG_SUM: fk = F_SUM, fa = add_slot(S_CNT_DEC, c); break;
        case HSG_MIN:
        case HSG_MAX: {
          const int op = g.kind == HSG_MIN ? S_TIE_MIN : S_TIE_MAX;
          fk = g.kind == HSG_MIN ? F_MIN : F_MAX;
          fa = add_slot(op, c);
          if (fa >= 0) prog.slot_aux[fa] = a;  // the MIN / MAX slot it breaks ties of
          break;
        }
        case HSG_LAST: fk = F_LAST, fa = add_slot(S_LAST_FORM, c); break;
        default: break;
      }
      if (fa < 0) return fail(err, HSG_E_INVALID, "too many state slots");
    }
    prog.form_kind[j] = fk;
    prog.form_a[j] = fa;
  }
  prog.n_out = (int)aggs.size();
  for (int s = 0; s < prog.n_slots; ++s) prog.ties |= slot_is_tie(prog.slot_op[s]) ? 1 : 0;
  // the per-record state projection (hsg_internal.h fin_*): the slots the
  // outputs read, plus the form word, when that is smaller than the state
  bool used[kMaxSlots] = {};
  bool forms_any = false;
  for (int j = 0; j < prog.n_out; ++j) {
    used[prog.out_a[j]] = true;
    if (prog.out_kind[j] == O_AVG_I || prog.out_kind[j] == O_AVG_F) used[prog.out_b[j]] = true;
    forms_any |= prog.form_kind[j] != F_NONE;
  }
  int nf = 0;
  for (int s = 0; s < prog.n_slots; ++s)
    if (used[s]) prog.fin_slot[nf++] = s;
  if (nf + (forms_any ? 1 : 0) < prog.n_slots) {
    prog.fin_n = nf;
    prog.fin_form = forms_any ? 1 : 0;
  } else {
    prog.fin_n = prog.n_slots;
    prog.fin_form = 0;
    for (int s = 0; s < prog.n_slots; ++s) prog.fin_slot[s] = s;
  }
  return HSG_OK;
}

}  // namespace hsg

// ---------------------------------------------------------------------------
// WHERE / HAVING program (include/hstream_gpu.h hsg_where_ins): host type check
// ---------------------------------------------------------------------------
static int validate_config(const hsg_op_config *c, std::string &err, int32_t agg_cols = -1);

namespace hsg {

static bool fn_exact(int32_t fn) {
  return fn == HSG_FN_ABS || fn == HSG_FN_CEIL || fn == HSG_FN_FLOOR || fn == HSG_FN_ROUND || fn == HSG_FN_SIGN ||
         fn == HSG_FN_SQRT;
}

int prog_fn_class(const hsg_where_ins *prog, int32_t n) {
  int fc = 0;
  for (int pc = 0; prog && pc < n; ++pc)
    if (prog[pc].op == HSG_W_FN) fc = std::max(fc, fn_exact(prog[pc].arg) ? 1 : 2);
  return fc;
}

// The static typing of one value instruction -- COL, I64, F64, ADD, SUB, MUL,
// FN -- as the device carries it (hsg_pred.h), written once for the three
// checkers: the values it pops (the top `pops` entries of is_f64[0 .. depth)
// are its operands), with f64 the type of the value it pushes; -1: `in` is no
// value instruction; -2: a fault, its text in msg. With fewer than `pops`
// entries f64 is not set: the caller reports the underflow.
static int value_ins_type(const hsg_where_ins &in, const int32_t *col_types, int32_t n_cols, const bool *is_f64,
                          int depth, bool &f64, std::string &msg) {
  f64 = false;
  int pops = 0;
  switch (in.op) {
    case HSG_W_COL:
      if (in.arg < 0 || in.arg >= n_cols) {
        msg = "column " + std::to_string(in.arg) + " out of range";
        return -2;
      }
      if (col_types[in.arg] != HSG_I64 && col_types[in.arg] != HSG_F64) {
        msg = "bad column type";
        return -2;
      }
      f64 = col_types[in.arg] == HSG_F64;
      return 0;
    case HSG_W_I64: return 0;
    case HSG_W_F64:
      if (!(in.imm.f - in.imm.f == 0.0)) {
        msg = "f64 constant is not finite";
        return -2;
      }
      f64 = true;
      return 0;
    case HSG_W_ADD: case HSG_W_SUB: case HSG_W_MUL: pops = 2; break;
    case HSG_W_FN:
      if (in.arg < 0 || in.arg >= HSG_FN_COUNT) {
        msg = "bad function " + std::to_string(in.arg);
        return -2;
      }
      pops = 1;
      break;
    default: return -1;
  }
  if (depth < pops) return pops;
  // value value -> value: i64 only when both are
  for (int k = 0; k < pops; ++k) f64 |= is_f64[depth - 1 - k];
  if (in.op == HSG_W_FN) {
    // ABS / CEIL / FLOOR / ROUND keep the operand's type, SIGN is an i64, the rest f64
    if (in.arg == HSG_FN_SIGN) f64 = false;
    else if (in.arg != HSG_FN_ABS && in.arg != HSG_FN_CEIL && in.arg != HSG_FN_FLOOR && in.arg != HSG_FN_ROUND) f64 = true;
  }
  return pops;
}

// What a compiler needs of a program beside its result (prog_walk).
struct ProgFacts {
  int fn_class = 0;       // prog_fn_class
  // a function can give the error value or a literal-form bit of its own
  // (MapPlan::fn_valid): any but ABS / CEIL / FLOOR / ROUND / SIGN of an i64,
  // which is total and clears or keeps the bit
  bool fn_valid = false;
};

// The static walk of a program's stack, written once for every checker and
// compiler: each instruction's operands are there, values where values are
// wanted and bools where bools are, and the program leaves one result, a bool
// (want_bool: a predicate; the comparisons and connectives are then
// instructions too) or a value, whose type res_f64 takes. `pre` opens every
// message: "where: ", "having: ", "map: expr j: ". facts may be null.
static int prog_walk(const std::string &pre, bool want_bool, const hsg_where_ins *prog, int32_t n,
                     const int32_t *col_types, int32_t n_cols, bool &res_f64, std::string &err,
                     ProgFacts *facts = nullptr) {
  enum { K_VALUE = 0, K_BOOL = 1 };
  int kind[HSG_WHERE_MAX_DEPTH];
  bool is_f64[HSG_WHERE_MAX_DEPTH];  // a value's static type, as the device carries it (hsg_pred.h)
  int depth = 0;
  auto at = [&](int pc) { return pre + "instruction " + std::to_string(pc) + ": "; };
  for (int pc = 0; pc < n; ++pc) {
    const hsg_where_ins &in = prog[pc];
    int want = K_VALUE, gives = K_VALUE;
    bool f64 = false;
    std::string msg;
    int pops = value_ins_type(in, col_types, n_cols, is_f64, depth, f64, msg);
    if (pops == -2) return fail(err, HSG_E_INVALID, at(pc) + msg);
    if (pops == -1 && !want_bool)
      return fail(err, HSG_E_INVALID, at(pc) + "opcode " + std::to_string(in.op) + " is not a value instruction");
    if (pops == -1) switch (in.op) {
      case HSG_W_EQ: case HSG_W_NE: case HSG_W_LT: case HSG_W_GT: case HSG_W_LE: case HSG_W_GE:
        pops = 2, gives = K_BOOL;
        break;
      case HSG_W_BETWEEN: pops = 3, gives = K_BOOL; break;
      case HSG_W_AND: case HSG_W_OR: pops = 2, want = K_BOOL, gives = K_BOOL; break;
      case HSG_W_NOT: pops = 1, want = K_BOOL, gives = K_BOOL; break;
      default: return fail(err, HSG_E_INVALID, at(pc) + "bad opcode " + std::to_string(in.op));
    }
    if (depth < pops) return fail(err, HSG_E_INVALID, at(pc) + "stack underflow");
    for (int k = 0; k < pops; ++k)
      if (kind[depth - 1 - k] != want)
        return fail(err, HSG_E_INVALID,
                    at(pc) + (want == K_VALUE ? "a bool used as a value" : "a value used as a bool"));
    if (facts && in.op == HSG_W_FN) {
      facts->fn_class = std::max(facts->fn_class, fn_exact(in.arg) ? 1 : 2);
      facts->fn_valid |= is_f64[depth - 1] || in.arg == HSG_FN_SQRT || !fn_exact(in.arg);
    }
    depth -= pops;
    if (depth >= HSG_WHERE_MAX_DEPTH)
      return fail(err, HSG_E_INVALID, at(pc) + "stack deeper than " + std::to_string(HSG_WHERE_MAX_DEPTH));
    is_f64[depth] = gives == K_VALUE && f64;
    kind[depth++] = gives;
  }
  if (depth != 1)
    return fail(err, HSG_E_INVALID,
                pre + std::to_string(depth) + (want_bool ? " results" : " values") + " left on the stack, not one");
  if (want_bool && kind[0] != K_BOOL)
    return fail(err, HSG_E_INVALID,
                pre + "the program leaves a value, not a bool (" + (is_f64[0] ? "an f64" : "an i64") + " value)");
  res_f64 = is_f64[0];
  return HSG_OK;
}

// (`what`: "where" over the value columns, "having" over the aggregate outputs)
static int prog_check(const std::string &what, const hsg_where_ins *prog, int32_t n, const int32_t *col_types,
                      int32_t n_cols, int32_t max_cols, std::string &err) {
  if (!prog) return fail(err, HSG_E_INVALID, what + ": null program");
  if (n < 1 || n > HSG_WHERE_MAX_INS)
    return fail(err, HSG_E_INVALID, what + ": program length " + std::to_string(n) + " outside 1.." +
                                        std::to_string(HSG_WHERE_MAX_INS));
  if (n_cols < 0 || n_cols > max_cols || (n_cols > 0 && !col_types))
    return fail(err, HSG_E_INVALID, what + ": bad value columns (max " + std::to_string(max_cols) + ")");
  bool res_f64;
  return prog_walk(what + ": ", true, prog, n, col_types, n_cols, res_f64, err);
}

int where_check(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, std::string &err) {
  return prog_check("where", prog, n, col_types, n_cols, kMaxCols, err);
}

void having_types(const hsg_op_config *cfg, int32_t *types) {
  for (int j = 0; j < cfg->n_aggs; ++j) {
    const hsg_agg &g = cfg->aggs[j];
    if (g.kind == HSG_COUNT_ALL || g.kind == HSG_COUNT) types[j] = HSG_I64;
    else if (g.kind == HSG_AVG) types[j] = HSG_F64;
    else types[j] = cfg->col_types[g.column];
  }
}

int having_check(const hsg_where_ins *prog, int32_t n, const hsg_op_config *cfg, std::string &err) {
  int rc = validate_config(cfg, err);
  if (rc != HSG_OK) return rc;
  if (cfg->n_aggs > kMaxAggs) return fail(err, HSG_E_INVALID, "having: more than 16 aggregates");
  int32_t types[kMaxAggs];
  having_types(cfg, types);
  return prog_check("having", prog, n, types, cfg->n_aggs, kMaxAggs, err);
}

// (also the HAVING program over the aggregate outputs' types: up to kMaxAggs columns)
void where_compile(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, WhereProg &out) {
  memset(&out, 0, sizeof(out));
  out.n = n;
  out.fn_class = (uint32_t)prog_fn_class(prog, n);
  for (int c = 0; c < n_cols; ++c)
    if (col_types[c] == HSG_F64) out.f64 |= 1u << c;
  for (int pc = 0; pc < n; ++pc) {
    out.ins[pc] = prog[pc];
    if (prog[pc].op == HSG_W_COL) out.cols |= 1u << prog[pc].arg;
  }
}

// ---- computed columns: the map's value programs ------------------------------
int map_check(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols, int32_t *out_types,
              std::string &err) {
  if (!exprs) return fail(err, HSG_E_INVALID, "map: null expressions");
  if (n_exprs < 1 || n_exprs > HSG_MAP_MAX_EXPRS)
    return fail(err, HSG_E_INVALID, "map: " + std::to_string(n_exprs) + " expressions outside 1.." +
                                        std::to_string(HSG_MAP_MAX_EXPRS));
  if (n_cols < 0 || n_cols > kMaxCols || (n_cols > 0 && !col_types))
    return fail(err, HSG_E_INVALID, "map: bad value columns (max " + std::to_string(kMaxCols) + ")");
  int64_t total = 0;
  for (int j = 0; j < n_exprs; ++j) {
    const std::string what = "map: expr " + std::to_string(j) + ": ";
    const hsg_map_expr &x = exprs[j];
    if (!x.prog) return fail(err, HSG_E_INVALID, what + "null program");
    if (x.n < 1 || x.n > HSG_MAP_MAX_INS)
      return fail(err, HSG_E_INVALID, what + "program length " + std::to_string(x.n) + " outside 1.." +
                                          std::to_string(HSG_MAP_MAX_INS));
    if (x.flags & ~HSG_MAP_STRICT) return fail(err, HSG_E_INVALID, what + "bad flags");
    total += x.n;
    if (total > HSG_MAP_MAX_INS)
      return fail(err, HSG_E_INVALID, what + std::to_string(total) + " instructions with the expressions before it, more than " +
                                          std::to_string(HSG_MAP_MAX_INS));
    bool res_f64;
    const int rc = prog_walk(what, false, x.prog, x.n, col_types, n_cols, res_f64, err);
    if (rc != HSG_OK) return rc;
    if (out_types) out_types[j] = res_f64 ? HSG_F64 : HSG_I64;
  }
  return HSG_OK;
}

void map_compile(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols, bool forms,
                 const WhereProg &where, MapProg &out, MapPlan &plan) {
  memset(&out, 0, sizeof(out));
  plan = MapPlan();
  out.where = where;
  out.cols = where.n ? where.cols : 0;
  out.forms = forms ? 1u : 0u;
  for (int c = 0; c < n_cols; ++c)
    if (col_types[c] == HSG_F64) out.f64 |= 1u << c;
  plan.n_exprs = n_exprs;
  plan.keys = where.n != 0;
  plan.fn_class = where.n ? (int32_t)where.fn_class : 0;
  for (int j = 0; j < n_exprs; ++j) {
    const hsg_map_expr &x = exprs[j];
    const bool strict = (x.flags & HSG_MAP_STRICT) != 0;
    const bool alias = x.n == 1 && x.prog[0].op == HSG_W_COL;
    plan.alias[j] = alias ? x.prog[0].arg : -1;
    plan.ocol[j] = alias ? -1 : plan.n_out++;
    plan.keys |= strict;
    for (int pc = 0; pc < x.n; ++pc) {
      const hsg_where_ins &in = x.prog[pc];
      if (in.op == HSG_W_COL) plan.reads[j] |= 1u << in.arg;
      if (in.op == HSG_W_F64 && in.imm.f != __builtin_trunc(in.imm.f)) plan.const_form[j] = true;
    }
    ProgFacts facts;
    bool res_f64;
    std::string ignored;  // (checked)
    prog_walk("", false, x.prog, x.n, col_types, n_cols, res_f64, ignored, &facts);
    plan.fn_class = std::max(plan.fn_class, (int32_t)facts.fn_class);
    plan.fn_valid[j] = facts.fn_valid;
    if (alias && !strict) continue;  // the caller's column as it is: nothing to run
    for (int pc = 0; pc < x.n; ++pc) {
      hsg_where_ins in = x.prog[pc];
      // the literal-form bit of a constant: an F64 that is not integral (ops that keep forms only)
      if (in.op == HSG_W_I64) in.arg = 0;
      if (in.op == HSG_W_F64) in.arg = forms && in.imm.f != __builtin_trunc(in.imm.f) ? 1 : 0;
      out.ins[out.n_ins++] = in;
    }
    out.cols |= plan.reads[j];
    out.end[out.n_runs] = out.n_ins;
    out.out[out.n_runs] = plan.ocol[j];
    if (strict) out.strict |= 1u << out.n_runs;
    ++out.n_runs;
  }
}

// ---- scalar SELECT: the three programs of a select op ---------------------------
int select_check(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                 const hsg_where_ins *having, int32_t n_having, const int32_t *col_types, int32_t n_cols,
                 int32_t *out_types, std::string &err) {
  if (n_cols < 0 || n_cols > kMaxCols || (n_cols > 0 && !col_types))
    return fail(err, HSG_E_INVALID, "select: bad value columns (max " + std::to_string(kMaxCols) + ")");
  for (int c = 0; c < n_cols; ++c)
    if (col_types[c] != HSG_I64 && col_types[c] != HSG_F64) return fail(err, HSG_E_INVALID, "select: bad column type");
  if (n_where < 0 || n_having < 0) return fail(err, HSG_E_INVALID, "select: negative program length");
  int rc = n_where ? where_check(where, n_where, col_types, n_cols, err) : HSG_OK;
  if (rc != HSG_OK) return rc;
  int32_t types[HSG_MAP_MAX_EXPRS] = {};
  // (no expression at all is SELECT *: the rows carry src_index only)
  if (n_exprs != 0) rc = map_check(exprs, n_exprs, col_types, n_cols, types, err);
  if (rc != HSG_OK) return rc;
  if (n_having) rc = prog_check("having", having, n_having, types, n_exprs, HSG_MAP_MAX_EXPRS, err);
  if (rc != HSG_OK) return rc;
  for (int j = 0; out_types && j < n_exprs; ++j) out_types[j] = types[j];
  return HSG_OK;
}

int select_compile(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                   const hsg_where_ins *having, int32_t n_having, const int32_t *col_types, int32_t n_cols,
                   const int32_t *expr_types, bool forms, SelectProg &out) {
  memset(&out, 0, sizeof(out));
  WhereProg wp;
  memset(&wp, 0, sizeof(wp));
  if (n_where) where_compile(where, n_where, col_types, n_cols, wp);
  // every expression strict: map_compile then keeps each one, aliases included, as a run of its own
  hsg_map_expr strict[HSG_MAP_MAX_EXPRS];
  for (int j = 0; j < n_exprs; ++j) {
    strict[j] = exprs[j];
    strict[j].flags = HSG_MAP_STRICT;
  }
  MapPlan plan;
  map_compile(strict, n_exprs, col_types, n_cols, forms, wp, out.m, plan);
  out.n_exprs = n_exprs;
  for (int j = 0; j < n_exprs; ++j)
    if (expr_types[j] == HSG_F64) out.ef64 |= 1u << j;
  int fc = plan.fn_class;
  if (n_having) {
    where_compile(having, n_having, expr_types, n_exprs, out.having);
    fc = std::max(fc, (int)out.having.fn_class);
  }
  return fc;
}

}  // namespace hsg

template <class F>
static int checked_message(F check, char *err, size_t err_len) {
  try {
    std::string msg;
    const int rc = check(msg);
    if (err && err_len) {
      const size_t k = msg.size() < err_len - 1 ? msg.size() : err_len - 1;
      memcpy(err, msg.data(), k);
      err[k] = 0;
    }
    return rc;
  } catch (...) {
    return HSG_E_OOM;
  }
}

extern "C" int hsg_map_check(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols,
                             int32_t *out_types, char *err, size_t err_len) {
  return checked_message(
      [&](std::string &msg) { return map_check(exprs, n_exprs, col_types, n_cols, out_types, msg); }, err, err_len);
}

extern "C" int hsg_select_check(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                                const hsg_where_ins *having, int32_t n_having, const int32_t *col_types,
                                int32_t n_cols, char *err, size_t err_len) {
  return checked_message(
      [&](std::string &msg) {
        return select_check(where, n_where, exprs, n_exprs, having, n_having, col_types, n_cols, nullptr, msg);
      },
      err, err_len);
}

extern "C" int hsg_where_check(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, char *err,
                               size_t err_len) {
  return checked_message([&](std::string &msg) { return where_check(prog, n, col_types, n_cols, msg); }, err, err_len);
}

extern "C" int hsg_having_check(const hsg_where_ins *prog, int32_t n, const hsg_op_config *cfg, char *err,
                                size_t err_len) {
  return checked_message([&](std::string &msg) { return having_check(prog, n, cfg, msg); }, err, err_len);
}

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
struct hsg_engine {
  int device = 0;
  int rank = 0;
  int nranks = 1;
  uint64_t batch_cap = 0;
  std::string err;
  std::mutex mu;  // guards the engine communicator (op creation splits it)
  Comm *comm = nullptr;
};

extern "C" int hsg_comm_unique_id(uint8_t *out, size_t len) {
  try {
    if (!out || len < HSG_COMM_ID_BYTES) return HSG_E_INVALID;
    return comm_unique_id(out);
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_engine_create(const hsg_engine_config *cfg, hsg_engine **out) {
  try {
    if (!cfg || !out) return HSG_E_INVALID;
    *out = nullptr;
    if (cfg->nranks < 1 || cfg->rank < 0 || cfg->rank >= cfg->nranks) return HSG_E_INVALID;
    if (cfg->nranks > 1 && !cfg->comm_id) return HSG_E_INVALID;
    if (cfg->batch_capacity == 0) return HSG_E_INVALID;
    hsg_engine *e = new (std::nothrow) hsg_engine();
    if (!e) return HSG_E_OOM;
    int dev = cfg->device;
    if (dev < 0) {
      if (hipGetDevice(&dev) != hipSuccess) { delete e; return HSG_E_DEVICE; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || dev >= ndev) { delete e; return HSG_E_DEVICE; }
    if (hipSetDevice(dev) != hipSuccess) { delete e; return HSG_E_DEVICE; }
    e->device = dev;
    e->rank = cfg->rank;
    e->nranks = cfg->nranks;
    e->batch_cap = cfg->batch_capacity;
    if (cfg->transport != HSG_TRANSPORT_RCCL && cfg->transport != HSG_TRANSPORT_HOST) { delete e; return HSG_E_INVALID; }
    if (cfg->nranks > 1 || cfg->comm_id) {
      int rc = comm_create(cfg->comm_id, cfg->rank, cfg->nranks, dev, cfg->transport, cfg->batch_capacity, &e->comm,
                           e->err);
      if (rc != HSG_OK) { delete e; return rc; }
    }
    *out = e;
    return HSG_OK;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" void hsg_engine_destroy(hsg_engine *e) {
  if (!e) return;
  try {
    hipSetDevice(e->device);
    if (e->comm) comm_destroy(e->comm);
  } catch (...) {
  }
  delete e;
}

extern "C" const char *hsg_engine_last_error(const hsg_engine *e) { return e ? e->err.c_str() : "null engine"; }

// testing knobs (include/hstream_gpu.h): process-wide, read at op creation
static std::atomic<int64_t> g_knob_xpart{-1}, g_knob_arena{0}, g_knob_xclassic{0};

namespace hsg {
int64_t testing_knob(int knob) {
  switch (knob) {
    case HSG_KNOB_XPART_LOG2: return g_knob_xpart.load();
    case HSG_KNOB_SESS_ARENA_MIN: return g_knob_arena.load();
    case HSG_KNOB_X_CLASSIC: return g_knob_xclassic.load();
    default: return 0;
  }
}
}  // namespace hsg

extern "C" int hsg_testing_set_knob(int32_t knob, int64_t value) {
  switch (knob) {
    case HSG_KNOB_XPART_LOG2:
      if (value < -1 || value > 6) return HSG_E_INVALID;
      g_knob_xpart.store(value);
      return HSG_OK;
    case HSG_KNOB_SESS_ARENA_MIN:
      if (value < 0) return HSG_E_INVALID;
      g_knob_arena.store(value);
      return HSG_OK;
    case HSG_KNOB_X_CLASSIC:
      if (value < 0 || value > 1) return HSG_E_INVALID;
      g_knob_xclassic.store(value);
      return HSG_OK;
    default: return HSG_E_INVALID;
  }
}

// ---------------------------------------------------------------------------
// op
// ---------------------------------------------------------------------------
// One queued asynchronous push: the batch descriptor is copied (the caller's
// struct may live on its stack); the arrays it points to are the caller's.
struct AsyncJob {
  hsg_batch b;
  std::vector<const void *> cols;
  std::vector<const uint8_t *> valid;
  int64_t *wm = nullptr;
  hsg_done_fn done = nullptr;
  void *ctx = nullptr;
  int staged_set = -1;  // host arrays already queued for H2D (op_prestage)
};

struct hsg_op {
  hsg_engine *eng = nullptr;
  hsg_op_config cfg;
  std::vector<int32_t> col_types;  // the user's value columns
  std::vector<hsg_agg> aggs;
  int32_t user_cols = 0;           // value columns of the caller's batches (= cfg.n_cols)
  Program prog;
  OpDevice dev;  // every HBM buffer + stream + events (hsg_ops.h)
  // Sharded ops own a communicator split from the engine's at creation, so
  // pushes of distinct ops never share RCCL call ordering (ranks may run their
  // queries' pushes in any interleaving) and need no engine-wide lock.
  Comm *comm = nullptr;
  std::string err;
  uint64_t pending = 0;
  uint64_t state_rows = 0;
  uint32_t batch_id = 0;
  uint64_t rec_base = 0;
  hsg_stats stats;
  hsg_map_stats map_stats = {};  // the map's counters (hsg_op_map_stats)
  bool select = false;           // a select op (hsg_op_create_select): no group key, no state
  hsg_select_stats sel_stats = {};
  // asynchronous pushes (hsg_push_batch_async): one completion thread per op
  std::mutex qmu;
  std::condition_variable qcv;
  std::deque<AsyncJob> queue;
  bool busy = false;       // a job is running
  bool stopping = false;
  int async_rc = HSG_OK;   // first failure since the last hsg_op_wait
  std::thread worker;
  int next_set = 0;        // staging set of the next prestaged batch
};

static int push_sync(hsg_op *op, const hsg_batch *b, int64_t *inout_watermark, int staged_set = -1);

// Queue the H2D copies of a queued host batch so that they
// overlap the batch before it; the sets alternate, so the set a prestage
// fills was last read by a push that has completed (pushes are synchronous on
// the op's completion thread). Failure only means the push stages itself.
static void prestage_job(hsg_op *op, AsyncJob &job) {
  if (job.staged_set >= 0 || job.b.mem != HSG_MEM_HOST || job.b.n == 0) return;
  if (job.b.n > op->eng->batch_cap || job.b.n_cols != op->user_cols || !job.b.key_id || !job.b.ts)
    return;  // push_sync reports it
  hsg_batch b = job.b;
  b.cols = job.cols.empty() ? nullptr : job.cols.data();
  b.valid = job.valid.empty() ? nullptr : job.valid.data();
  for (int c = 0; c < b.n_cols; ++c)
    if (!b.cols || !b.cols[c]) return;
  if (hipSetDevice(op->eng->device) != hipSuccess) return;
  std::string err;
  const int set = op->next_set;
  if (op_prestage(op->dev, &b, set, err) == HSG_OK) {
    job.staged_set = set;
    op->next_set ^= 1;
  }
}

// Wait for the op's queued asynchronous pushes; returns (and clears) the first
// failure among them.
static int drain_async(hsg_op *op) {
  std::unique_lock<std::mutex> lk(op->qmu);
  op->qcv.wait(lk, [&] { return op->queue.empty() && !op->busy; });
  int rc = op->async_rc;
  op->async_rc = HSG_OK;
  return rc;
}

// Same wait, keeping a failure for the next hsg_op_wait / hsg_push_batch.
static void wait_idle(const hsg_op *cop) {
  hsg_op *op = const_cast<hsg_op *>(cop);
  std::unique_lock<std::mutex> lk(op->qmu);
  op->qcv.wait(lk, [&] { return op->queue.empty() && !op->busy; });
}

static void async_loop(hsg_op *op) {
  std::unique_lock<std::mutex> lk(op->qmu);
  for (;;) {
    op->qcv.wait(lk, [&] { return op->stopping || !op->queue.empty(); });
    if (op->queue.empty()) return;  // stopping with nothing left
    AsyncJob job = std::move(op->queue.front());
    op->queue.pop_front();
    op->busy = true;
    // the next queued job stays in the deque (only this thread pops it, and
    // push_back keeps references to elements valid)
    AsyncJob *next = op->queue.empty() ? nullptr : &op->queue.front();
    lk.unlock();
    prestage_job(op, job);
    if (next) prestage_job(op, *next);
    job.b.cols = job.cols.empty() ? nullptr : job.cols.data();
    job.b.valid = job.valid.empty() ? nullptr : job.valid.data();
    const int rc = push_sync(op, &job.b, job.wm, job.staged_set);
    if (job.done) job.done(job.ctx, rc);
    lk.lock();
    if (rc != HSG_OK && op->async_rc == HSG_OK) op->async_rc = rc;
    op->busy = false;
    op->qcv.notify_all();
  }
}

// (agg_cols: what aggs[].column indexes, the map's expressions of a mapped op; -1: the batch's columns)
static int validate_config(const hsg_op_config *c, std::string &err, int32_t agg_cols) {
  if (!c) return fail(err, HSG_E_INVALID, "null config");
  if (c->window_kind < HSG_TUMBLING || c->window_kind > HSG_UNWINDOWED) return fail(err, HSG_E_INVALID, "bad window_kind");
  if (c->emit_mode < HSG_EMIT_PER_RECORD || c->emit_mode > HSG_EMIT_NONE) return fail(err, HSG_E_INVALID, "bad emit_mode");
  if (c->window_kind == HSG_TUMBLING || c->window_kind == HSG_HOPPING) {
    if (c->size_ms <= 0) return fail(err, HSG_E_INVALID, "size_ms must be > 0");
    if (c->window_kind == HSG_HOPPING && c->advance_ms <= 0) return fail(err, HSG_E_INVALID, "advance_ms must be > 0");
  }
  if (c->window_kind == HSG_SESSION && c->gap_ms < 0) return fail(err, HSG_E_INVALID, "gap_ms must be >= 0");
  if (c->n_aggs <= 0 || !c->aggs) return fail(err, HSG_E_INVALID, "no aggregates");
  if (c->n_cols < 0 || c->n_cols > kMaxCols || (c->n_cols > 0 && !c->col_types))
    return fail(err, HSG_E_INVALID, "bad value columns (max 8)");
  for (int i = 0; i < c->n_cols; ++i)
    if (c->col_types[i] != HSG_I64 && c->col_types[i] != HSG_F64) return fail(err, HSG_E_INVALID, "bad column type");
  for (int j = 0; j < c->n_aggs; ++j) {
    const hsg_agg &g = c->aggs[j];
    if (g.kind < HSG_COUNT_ALL || g.kind > HSG_LAST) return fail(err, HSG_E_INVALID, "bad aggregate kind");
    if (g.kind != HSG_COUNT_ALL && (g.column < 0 || g.column >= (agg_cols >= 0 ? agg_cols : c->n_cols)))
      return fail(err, HSG_E_INVALID, "aggregate column out of range");
  }
  return HSG_OK;
}

uint64_t hsg_windows_per_record(const hsg_op_config &c) {
  // ceil(size / advance); (size + advance - 1) would pass INT64_MAX for a size near it
  if (c.window_kind == HSG_HOPPING) return (uint64_t)((c.size_ms - 1) / c.advance_ms + 1);
  return 1;
}

// hsg_op_create is the n_exprs == 0, n == 0, n_having == 0 case.
extern "C" int hsg_op_create_mapped(hsg_engine *eng, const hsg_op_config *cfg, const hsg_map_expr *exprs, int32_t n_exprs,
                                    const hsg_where_ins *where, int32_t n, const hsg_where_ins *having,
                                    int32_t n_having, hsg_op **out) {
  try {
    if (!eng || !out) return HSG_E_INVALID;
    *out = nullptr;
    int rc = validate_config(cfg, eng->err, n_exprs != 0 ? n_exprs : -1);
    if (rc != HSG_OK) return rc;
    if (n != 0) {
      rc = where_check(where, n, cfg->col_types, cfg->n_cols, eng->err);
      if (rc != HSG_OK) return rc;
    }
    // the aggregates' columns and their types: the map's expressions, or the batch's columns
    int32_t mtypes[HSG_MAP_MAX_EXPRS];
    hsg_op_config acfg = *cfg;
    if (n_exprs != 0) {
      rc = map_check(exprs, n_exprs, cfg->col_types, cfg->n_cols, mtypes, eng->err);
      if (rc != HSG_OK) return rc;
      acfg.n_cols = n_exprs;
      acfg.col_types = mtypes;
    }
    if (n_having != 0) {
      rc = having_check(having, n_having, &acfg, eng->err);
      if (rc != HSG_OK) return rc;
      if (cfg->emit_mode == HSG_EMIT_NONE)
        return fail(eng->err, HSG_E_INVALID, "having: an op that emits no rows (HSG_EMIT_NONE) has nothing to filter");
    }
    hsg_op *op = new (std::nothrow) hsg_op();
    if (!op) return HSG_E_OOM;
    op->eng = eng;
    op->cfg = *cfg;
    op->col_types.assign(cfg->col_types, cfg->col_types + cfg->n_cols);
    op->aggs.assign(cfg->aggs, cfg->aggs + cfg->n_aggs);
    op->cfg.col_types = nullptr;
    op->cfg.aggs = nullptr;
    if (op->cfg.window_kind == HSG_TUMBLING) op->cfg.advance_ms = op->cfg.size_ms;
    memset(&op->stats, 0, sizeof(op->stats));
    // literal forms: extra slots read the literal bit of the valid bytes
    const bool forms = (cfg->flags & HSG_OPF_LITERAL_FORMS) != 0;
    // The kernels' columns. An op with a WHERE program aggregates only the
    // columns an aggregate reads: a column the program alone reads is part of
    // the batch (user_cols) and gone once the filter ran (op_device.cpp
    // stage_batch), so the op is, from there on, the op without it -- the same
    // slot program, kernel variants and words per record. Ops without a
    // program keep every column, read or not.
    std::vector<int32_t> itypes = op->col_types;
    std::vector<hsg_agg> iaggs = op->aggs;
    op->user_cols = cfg->n_cols;
    for (int c = 0; c < cfg->n_cols; ++c) op->dev.col_map[c] = c;
    if (n != 0) where_compile(where, n, cfg->col_types, cfg->n_cols, op->dev.where);
    if (n != 0 && n_exprs == 0) {
      int32_t to_internal[kMaxCols];
      int ni = 0;
      itypes.clear();
      for (int c = 0; c < cfg->n_cols; ++c) {
        bool read = false;
        for (const hsg_agg &g : op->aggs) read |= g.kind != HSG_COUNT_ALL && g.column == c;
        to_internal[c] = read ? ni : -1;
        if (!read) continue;
        op->dev.col_map[ni++] = c;
        itypes.push_back(op->col_types[c]);
      }
      for (hsg_agg &g : iaggs)
        if (g.kind != HSG_COUNT_ALL) g.column = to_internal[g.column];
      op->cfg.n_cols = ni;
    }
    if (n_exprs != 0) {
      // internal column j is expression j: the batch's columns, the ones only
      // the WHERE program reads included, are gone once the map ran (op_device.cpp
      // stage_map). The pass runs the WHERE program itself (dev.where stays empty).
      WhereProg wp = op->dev.where;
      memset(&op->dev.where, 0, sizeof(op->dev.where));
      map_compile(exprs, n_exprs, cfg->col_types, cfg->n_cols, forms, wp, op->dev.map_prog, op->dev.map);
      itypes.assign(mtypes, mtypes + n_exprs);
      iaggs = op->aggs;
      op->cfg.n_cols = n_exprs;
    }
    rc = build_program(op->cfg, itypes, iaggs, op->prog, eng->err, forms);
    if (rc != HSG_OK) { delete op; return rc; }
    op->dev.user_cols = cfg->n_cols;
    op->dev.forms = forms;
    if (n_having != 0) {
      // the changelog filter (k_having.hip): over the aggregate outputs, as the caller numbers them
      int32_t otypes[kMaxAggs];
      having_types(&acfg, otypes);
      where_compile(having, n_having, otypes, cfg->n_aggs, op->dev.having);
      op->dev.hv.n_aggs = cfg->n_aggs;
    }
    if (hipSetDevice(eng->device) != hipSuccess) { delete op; return HSG_E_DEVICE; }
    if (eng->comm) {
      // collective over the engine's ranks: every rank creates its sharded ops
      // in the same order (the same queries)
      std::lock_guard<std::mutex> lk(eng->mu);
      rc = comm_split(eng->comm, &op->comm, eng->err);
      if (rc != HSG_OK) {
        comm_destroy(op->comm);
        delete op;
        return rc;
      }
    }
    // a sharded op's ranks must all reach the agreement below, whatever
    // happened here: exceptions become a status
    try {
      rc = op_device_init(op->dev, op->cfg, op->prog, eng->batch_cap, eng->nranks, op->comm != nullptr,
                          hsg_windows_per_record(op->cfg), eng->err);
    } catch (const std::bad_alloc &) {
      rc = HSG_E_OOM;
      eng->err = "op_device_init: out of host memory";
    } catch (...) {
      rc = HSG_E_DEVICE;
      eng->err = "op_device_init: exception";
    }
    if (op->comm) {
      // the ranks agree on the creation: a rank whose shard failed (e.g. out
      // of memory) takes every rank's shard down with it, so no rank keeps an
      // op whose first exchange would wait forever on the missing one. The
      // failed shard's memory goes first, and the agreement's stream and
      // buffer were made with the communicator (comm_split), so nothing can
      // fail between here and the collective.
      if (rc != HSG_OK) op_device_free(op->dev);
      std::string aerr;
      const int arc = comm_agree(op->comm, rc, aerr);
      if (rc == HSG_OK && arc != HSG_OK) {
        rc = arc;
        eng->err = aerr;
      }
    }
    if (rc != HSG_OK) {
      op_device_free(op->dev);
      comm_destroy(op->comm);
      delete op;
      return rc;
    }
    op->map_stats.computed_cols = (uint32_t)op->dev.map.n_out;
    op->map_stats.aliased_cols = (uint32_t)(op->dev.map.n_exprs - op->dev.map.n_out);
    op->stats.state_slots = (uint64_t)op->prog.n_slots;
    op->stats.state_row_bytes = 8ull * (uint64_t)op->prog.n_slots + (cfg->window_kind == HSG_SESSION ? 16ull : 8ull);
    op->stats.table_slots = op->dev.cap;
    *out = op;
    return HSG_OK;
  } catch (const std::bad_alloc &) {
    return HSG_E_OOM;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

// A select op is an hsg_op with no aggregation behind it: to the calls that
// take rows it is an op of n_exprs outputs (cfg.n_aggs), to the sink an op of
// that many LAST columns, which print as its numbers do.
extern "C" int hsg_op_create_select(hsg_engine *eng, const hsg_select_config *cfg, const hsg_where_ins *where,
                                    int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                                    const hsg_where_ins *having, int32_t n_having, hsg_op **out) {
  try {
    if (!eng || !out) return HSG_E_INVALID;
    *out = nullptr;
    if (!cfg) return fail(eng->err, HSG_E_INVALID, "select: null config");
    if (cfg->flags & ~HSG_OPF_LITERAL_FORMS) return fail(eng->err, HSG_E_INVALID, "select: bad flags");
    int32_t types[HSG_MAP_MAX_EXPRS] = {};
    int rc = select_check(where, n_where, exprs, n_exprs, having, n_having, cfg->col_types, cfg->n_cols, types, eng->err);
    if (rc != HSG_OK) return rc;
    hsg_op *op = new (std::nothrow) hsg_op();
    if (!op) return HSG_E_OOM;
    op->eng = eng;
    op->select = true;
    memset(&op->cfg, 0, sizeof(op->cfg));
    op->cfg.window_kind = HSG_UNWINDOWED;
    op->cfg.emit_mode = HSG_EMIT_PER_RECORD;
    op->cfg.n_cols = cfg->n_cols;
    op->cfg.n_aggs = n_exprs;
    op->cfg.out_capacity = cfg->out_capacity;
    op->cfg.flags = cfg->flags;
    op->col_types.assign(cfg->col_types, cfg->col_types + cfg->n_cols);
    op->user_cols = cfg->n_cols;
    memset(&op->stats, 0, sizeof(op->stats));
    memset(&op->prog, 0, sizeof(op->prog));
    const bool forms = (cfg->flags & HSG_OPF_LITERAL_FORMS) != 0;
    op->prog.n_out = n_exprs;
    for (int j = 0; j < n_exprs; ++j) {
      op->aggs.push_back(hsg_agg{HSG_LAST, j});
      op->prog.out_kind[j] = types[j] == HSG_F64 ? O_F64 : O_I64;
      op->prog.form_kind[j] = forms ? F_LAST : F_NONE;
    }
    OpDevice &d = op->dev;
    d.is_select = true;
    d.forms = forms;
    d.sel_fc = select_compile(where, n_where, exprs, n_exprs, having, n_having, cfg->col_types, cfg->n_cols, types, forms, d.sel);
    if (hipSetDevice(eng->device) != hipSuccess) { delete op; return HSG_E_DEVICE; }
    // local on a sharded engine too: no communicator, each rank filters its own slice
    rc = select_device_init(d, cfg->n_cols, cfg->col_types, n_exprs, eng->batch_cap, cfg->out_capacity, eng->err);
    if (rc != HSG_OK) {
      op_device_free(d);
      delete op;
      return rc;
    }
    *out = op;
    return HSG_OK;
  } catch (const std::bad_alloc &) {
    return HSG_E_OOM;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_op_select_stats(const hsg_op *op, hsg_select_stats *out) {
  if (!op || !out || !op->select) return HSG_E_INVALID;
  wait_idle(op);
  *out = op->sel_stats;
  return HSG_OK;
}

extern "C" int hsg_op_create_filtered(hsg_engine *eng, const hsg_op_config *cfg, const hsg_where_ins *where, int32_t n,
                                      const hsg_where_ins *having, int32_t n_having, hsg_op **out) {
  return hsg_op_create_mapped(eng, cfg, nullptr, 0, where, n, having, n_having, out);
}

extern "C" int hsg_op_create_where(hsg_engine *eng, const hsg_op_config *cfg, const hsg_where_ins *where, int32_t n,
                                   hsg_op **out) {
  return hsg_op_create_filtered(eng, cfg, where, n, nullptr, 0, out);
}

extern "C" int hsg_op_create(hsg_engine *eng, const hsg_op_config *cfg, hsg_op **out) {
  return hsg_op_create_filtered(eng, cfg, nullptr, 0, nullptr, 0, out);
}

extern "C" void hsg_op_destroy(hsg_op *op) {
  if (!op) return;
  try {
    {
      std::lock_guard<std::mutex> lk(op->qmu);
      op->stopping = true;
    }
    op->qcv.notify_all();
    if (op->worker.joinable()) op->worker.join();  // runs what is queued first
    hipSetDevice(op->eng->device);
    op_device_free(op->dev);
    comm_destroy(op->comm);
  } catch (...) {
  }
  delete op;
}

extern "C" const char *hsg_last_error(const hsg_op *op) { return op ? op->err.c_str() : "null op"; }

extern "C" int hsg_op_reset(hsg_op *op) {
  try {
    if (!op) return HSG_E_INVALID;
    wait_idle(op);
    HIP_TRY(op, hipSetDevice(op->eng->device));
    int rc = op_device_reset(op->dev, op->cfg, op->prog, op->err);
    if (rc != HSG_OK) return rc;
    // counters in hsg_stats are cumulative since create; only the state goes
    op->pending = 0;
    op->state_rows = 0;
    op->rec_base = 0;
    op->stats.state_rows = 0;
    op->stats.pending_rows = 0;
    op->stats.spilled_rows = 0;
    return HSG_OK;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

static int validate_batch(hsg_op *op, const hsg_batch *b, const int64_t *inout_watermark) {
  if (!b || !inout_watermark) return fail(op->err, HSG_E_INVALID, "null batch or watermark");
  if (b->n_cols != op->user_cols) return fail(op->err, HSG_E_INVALID, "batch n_cols != op n_cols");
  if (b->mem != HSG_MEM_HOST && b->mem != HSG_MEM_DEVICE) return fail(op->err, HSG_E_INVALID, "bad batch mem");
  if (b->n > op->eng->batch_cap) return fail(op->err, HSG_E_CAPACITY, "batch larger than the engine's batch_capacity");
  // (a select op's batch may come without keys: every record is live)
  if (b->n && ((!b->key_id && !op->select) || !b->ts)) return fail(op->err, HSG_E_INVALID, "null key_id / ts");
  for (int c = 0; c < b->n_cols; ++c)
    if (b->n && (!b->cols || !b->cols[c])) return fail(op->err, HSG_E_INVALID, "null value column");
  // narrow transport (hsg_enc): ts as TS32 / TS16, i64 columns as I32, f64 columns as DEC32
  if (b->ts_enc != HSG_ENC_FULL && b->ts_enc != HSG_ENC_TS32 && b->ts_enc != HSG_ENC_TS16)
    return fail(op->err, HSG_E_INVALID, "bad ts_enc");
  if (b->ts_enc == HSG_ENC_TS16 && b->n && !b->ts_frames) return fail(op->err, HSG_E_INVALID, "TS16 without ts_frames");
  if (b->key_enc != HSG_ENC_FULL && b->key_enc != HSG_ENC_K16) return fail(op->err, HSG_E_INVALID, "bad key_enc");
  for (int c = 0; c < b->n_cols; ++c) {
    const int e = b->col_enc[c];
    const bool f64 = op->col_types[c] == HSG_F64;
    if (e != HSG_ENC_FULL && e != (f64 ? HSG_ENC_DEC32 : HSG_ENC_I32))
      return fail(op->err, HSG_E_INVALID, "bad col_enc for the column's type");
    if (e == HSG_ENC_DEC32 && b->col_scale[c] > 18) return fail(op->err, HSG_E_INVALID, "col_scale > 18");
  }
  return HSG_OK;
}

// The push itself (caller: hsg_push_batch, or the op's completion thread).
static int push_sync(hsg_op *op, const hsg_batch *b, int64_t *inout_watermark, int staged_set) {
  try {
    int rc = validate_batch(op, b, inout_watermark);
    if (rc != HSG_OK) return rc;
    HIP_TRY(op, hipSetDevice(op->eng->device));
    double t0 = now_ms();
    PushResult res;
    PushArgs args;
    args.batch = b;
    args.wm_in = *inout_watermark;
    args.batch_id = ++op->batch_id;
    args.rec_base = op->rec_base;
    args.pending = op->pending;
    args.comm = op->comm;
    args.rank = op->eng->rank;
    args.nranks = op->eng->nranks;
    args.staged_set = staged_set;
    rc = op_push(op->dev, op->cfg, op->prog, args, res, op->err);
    if (rc != HSG_OK && rc != HSG_E_RANGE && rc != HSG_E_OOM) return rc;
    if (op->dev.where.n) {
      // the filter's count came back with the scalars the push fetched
      const uint64_t seen = op->dev.h_sc->scratch[kWhereWord];
      res.where_dropped = seen - op->dev.where_seen;
      op->dev.where_seen = seen;
    }
    if (op->dev.map.n_exprs) {
      // the map pass keeps two cumulative 32-bit counts in the word: WHERE
      // drops below, strict map drops above (k_map.hip)
      const uint64_t seen = op->dev.h_sc->scratch[kWhereWord];
      res.where_dropped = (uint32_t)((uint32_t)seen - (uint32_t)op->dev.where_seen);
      op->dev.where_seen = (uint32_t)seen;
      op->map_stats.map_dropped = (uint32_t)((uint32_t)(seen >> 32) - op->dev.map_seen);
      op->map_stats.map_dropped_total += op->map_stats.map_dropped;
      op->dev.map_seen = (uint32_t)(seen >> 32);
    }
    if (op->dev.having.n && op->dev.hv_ran) {
      // the changelog filter's kept rows came back with the same fetch
      // (kHavingWord): the batch appended these, in order, from op->pending
      const uint64_t kept = op->dev.hv_kept < res.out_rows ? op->dev.hv_kept : res.out_rows;
      res.having_dropped = res.out_rows - kept;
      res.out_rows = kept;
    }
    if (op->select) {
      hsg_select_stats &ss = op->sel_stats;
      ss.where_dropped = op->dev.sel_dropped[0];
      ss.expr_dropped = op->dev.sel_dropped[1];
      ss.having_dropped = op->dev.sel_dropped[2];
      ss.emitted = res.out_rows;
      ss.where_dropped_total += ss.where_dropped;
      ss.expr_dropped_total += ss.expr_dropped;
      ss.having_dropped_total += ss.having_dropped;
      ss.emitted_total += ss.emitted;
    }
    // state was mutated: account for what happened even on OOM / RANGE
    *inout_watermark = res.wm_out;
    op->pending += res.out_rows;
    op->state_rows = res.state_rows;
    op->rec_base += res.global_records;
    op->stats.batches += 1;
    op->stats.records += b->n;
    op->stats.records_owned += res.owned;
    op->stats.pairs = res.pairs;
    op->stats.late_dropped = res.late;
    op->stats.touched = res.touched;
    op->stats.pairs_total += res.pairs;
    op->stats.touched_total += res.touched;
    op->stats.state_rows = op->state_rows;
    op->stats.spilled_rows = op->dev.spilled_rows;
    op->stats.spill_events = op->dev.spill_events;
    op->stats.table_slots = op->dev.cap;
    op->stats.grow_events = op->dev.grow_events;
    op->stats.lean_batches = op->dev.lean_batches;
    op->stats.direct_batches = op->dev.direct_batches;
    op->stats.replays = op->dev.replays;
    op->stats.overflow_rows = op->dev.ovf_rows;
    op->stats.overflow_rebuilds = op->dev.ovf_events;
    op->stats.pending_rows = op->pending;
    op->stats.where_dropped = res.where_dropped;
    op->stats.where_dropped_total += res.where_dropped;
    op->stats.having_dropped = res.having_dropped;
    op->stats.having_dropped_total += res.having_dropped;
    op->stats.last_batch_ms = now_ms() - t0;
    op->stats.agg_kernel_ms += res.agg_ms;
    op->stats.agg_kernel_launches += res.agg_launches;
    op->stats.exchange_ms += res.exchange_ms;
    op->stats.exchange_bytes += res.exchange_bytes;
    return rc;
  } catch (const std::bad_alloc &) {
    return HSG_E_OOM;
  } catch (...) {
    op->err = "unexpected exception";
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_push_batch(hsg_op *op, const hsg_batch *b, int64_t *inout_watermark) {
  if (!op) return HSG_E_INVALID;
  int rc = drain_async(op);
  if (rc != HSG_OK) return rc;
  return push_sync(op, b, inout_watermark);
}

extern "C" int hsg_push_batch_async(hsg_op *op, const hsg_batch *b, int64_t *inout_watermark, hsg_done_fn done,
                                    void *ctx) {
  try {
    if (!op) return HSG_E_INVALID;
    int rc = validate_batch(op, b, inout_watermark);
    if (rc != HSG_OK) return rc;
    AsyncJob job;
    job.b = *b;
    if (b->cols) job.cols.assign(b->cols, b->cols + b->n_cols);
    if (b->valid) job.valid.assign(b->valid, b->valid + b->n_cols);
    job.wm = inout_watermark;
    job.done = done;
    job.ctx = ctx;
    std::lock_guard<std::mutex> lk(op->qmu);
    if (op->stopping) return fail(op->err, HSG_E_INVALID, "op is being destroyed");
    if (!op->worker.joinable()) op->worker = std::thread(async_loop, op);
    op->queue.push_back(std::move(job));
    op->qcv.notify_all();
    return HSG_OK;
  } catch (const std::bad_alloc &) {
    return HSG_E_OOM;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_op_wait(hsg_op *op) {
  if (!op) return HSG_E_INVALID;
  return drain_async(op);
}

extern "C" int hsg_pending_rows(const hsg_op *op, uint64_t *n) {
  if (!op || !n) return HSG_E_INVALID;
  wait_idle(op);
  *n = op->pending;
  return HSG_OK;
}

static int check_rows(hsg_op *op, const hsg_rows *out) {
  if (!out) return fail(op->err, HSG_E_INVALID, "null rows");
  if (out->n_aggs != op->cfg.n_aggs) return fail(op->err, HSG_E_INVALID, "rows n_aggs != op n_aggs");
  if (out->mem != HSG_MEM_HOST && out->mem != HSG_MEM_DEVICE) return fail(op->err, HSG_E_INVALID, "bad rows mem");
  return HSG_OK;
}

extern "C" int hsg_op_set_changelog(hsg_op *op, const hsg_rows *dst) {
  try {
    if (!op) return HSG_E_INVALID;
    wait_idle(op);
    if (op->pending) return fail(op->err, HSG_E_INVALID, "set_changelog: drain the pending rows first");
    OpDevice &d = op->dev;
    if (!dst) {
      d.out = d.own_out;
      d.out_cap = d.own_out_cap;
      d.ext_out = false;
      return HSG_OK;
    }
    int rc = check_rows(op, dst);
    if (rc != HSG_OK) return rc;
    if (dst->mem != HSG_MEM_DEVICE) return fail(op->err, HSG_E_INVALID, "set_changelog: device columns only");
    if (!dst->key_id || !dst->win_start || !dst->win_end || !dst->src_index || dst->capacity == 0 ||
        (op->cfg.n_aggs && !dst->aggs))
      return fail(op->err, HSG_E_INVALID, "set_changelog: every column is required");
    OutCols o;
    memset(&o, 0, sizeof(o));
    o.key = dst->key_id;
    o.ws = dst->win_start;
    o.we = dst->win_end;
    o.src = dst->src_index;
    for (int j = 0; j < op->cfg.n_aggs; ++j) {
      if (!dst->aggs[j]) return fail(op->err, HSG_E_INVALID, "set_changelog: every column is required");
      o.agg[j] = (int64_t *)dst->aggs[j];
    }
    o.form = op->dev.forms ? dst->form : nullptr;  // (optional: rows then carry no forms)
    d.out = o;
    d.out_cap = dst->capacity;
    d.ext_out = true;
    return HSG_OK;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_drain(hsg_op *op, hsg_rows *out, uint64_t *n_out) {
  try {
    if (!op || !n_out) return HSG_E_INVALID;
    wait_idle(op);
    int rc = op->dev.ext_out && !out ? HSG_OK : check_rows(op, out);
    if (rc != HSG_OK) return rc;
    *n_out = op->pending;
    if (!op->dev.ext_out) {
      if (out->capacity < op->pending) return fail(op->err, HSG_E_CAPACITY, "drain: rows capacity < pending rows");
      HIP_TRY(op, hipSetDevice(op->eng->device));
      rc = op_copy_rows(op->dev, op->dev.out, 0, op->pending, op->cfg.n_aggs, out, op->err);
      if (rc != HSG_OK) return rc;
    }
    op->pending = 0;
    op->stats.pending_rows = 0;
    return HSG_OK;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_state_rows(hsg_op *op, uint64_t *n) {
  if (!op || !n) return HSG_E_INVALID;
  wait_idle(op);
  *n = op->state_rows;
  return HSG_OK;
}

extern "C" int hsg_dump_state(hsg_op *op, hsg_rows *out, uint64_t *n_out) {
  try {
    if (!op || !n_out) return HSG_E_INVALID;
    wait_idle(op);
    if (op->select) return fail(op->err, HSG_E_INVALID, "dump: a select op has no state");
    int rc = check_rows(op, out);
    if (rc != HSG_OK) return rc;
    *n_out = op->state_rows;
    if (out->capacity < op->state_rows) return fail(op->err, HSG_E_CAPACITY, "dump: rows capacity < state rows");
    HIP_TRY(op, hipSetDevice(op->eng->device));
    uint64_t n = 0;
    rc = op_dump(op->dev, op->cfg, op->prog, out, &n, op->err);
    *n_out = n;
    return rc;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_view_get(hsg_op *op, const uint32_t *key_ids, uint32_t n_keys, hsg_rows *out, uint64_t *n_out) {
  try {
    if (!op || !n_out) return HSG_E_INVALID;
    wait_idle(op);
    if (op->select) return fail(op->err, HSG_E_INVALID, "view_get: a select op has no state");
    int rc = check_rows(op, out);
    if (rc != HSG_OK) return rc;
    *n_out = 0;
    if (n_keys > HSG_VIEW_MAX_KEYS) return fail(op->err, HSG_E_INVALID, "view_get: more than HSG_VIEW_MAX_KEYS keys");
    if (n_keys && !key_ids) return fail(op->err, HSG_E_INVALID, "view_get: null key_ids");
    if (n_keys == 0) return HSG_OK;
    // duplicates count once; HSG_KEY_NONE names no group
    std::vector<uint32_t> keys(key_ids, key_ids + n_keys);
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    if (!keys.empty() && keys.back() == HSG_KEY_NONE) keys.pop_back();
    HIP_TRY(op, hipSetDevice(op->eng->device));
    return op_view_get(op->dev, op->cfg, op->prog, keys.data(), (uint32_t)keys.size(), out, n_out, op->err);
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_table_join(hsg_op *table, const hsg_probe *probe, hsg_rows *out, uint64_t *n_out) {
  try {
    hsg_op *op = table;
    if (!op || !n_out) return HSG_E_INVALID;
    wait_idle(op);
    if (op->select) return fail(op->err, HSG_E_INVALID, "table_join: a select op is no table");
    if (!probe) return fail(op->err, HSG_E_INVALID, "table_join: null probe");
    int rc = check_rows(op, out);
    if (rc != HSG_OK) return rc;
    *n_out = 0;
    // joinTableProcessor reads a KV store (getKVStateStore); window and session stores are none
    if (op->cfg.window_kind != HSG_UNWINDOWED)
      return fail(op->err, HSG_E_INVALID, "table_join: the table must be an unwindowed op");
    if (probe->reserved != 0) return fail(op->err, HSG_E_INVALID, "table_join: probe.reserved must be 0");
    if (probe->mem != HSG_MEM_HOST && probe->mem != HSG_MEM_DEVICE)
      return fail(op->err, HSG_E_INVALID, "table_join: bad probe mem");
    if (probe->n > op->eng->batch_cap)
      return fail(op->err, HSG_E_INVALID, "table_join: probe larger than the engine's batch_capacity");
    if (probe->n && !probe->key_id) return fail(op->err, HSG_E_INVALID, "table_join: null key_id");
    if (probe->n == 0) return HSG_OK;
    HIP_TRY(op, hipSetDevice(op->eng->device));
    return op_table_join(op->dev, op->cfg, op->prog, probe, out, n_out, op->err);
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_table_join_tile(void) { return (int)hsg::kTjTile; }

extern "C" int hsg_op_stats(const hsg_op *op, hsg_stats *out) {
  if (!op || !out) return HSG_E_INVALID;
  wait_idle(op);
  *out = op->stats;
  return HSG_OK;
}

extern "C" int hsg_op_map_stats(const hsg_op *op, hsg_map_stats *out) {
  if (!op || !out) return HSG_E_INVALID;
  wait_idle(op);
  *out = op->map_stats;
  return HSG_OK;
}

extern "C" int hsg_map_grid_threads(void) { return hsg::pass_grid(hsg::kPassMap, 0) * hsg::kMapThreads; }
extern "C" int hsg_map_grid_threads_fn(int fn_class) {
  return fn_class < 0 || fn_class > 2 ? 0 : hsg::pass_grid(hsg::kPassMap, fn_class) * hsg::kMapThreads;
}
extern "C" int hsg_prog_fn_class(const hsg_where_ins *prog, int32_t n) { return hsg::prog_fn_class(prog, n); }

namespace hsg {
// For the sink encoder (sink.cpp): the op's device and which changelog
// aggregate columns hold f64 bits.
int op_sink_info(const hsg_op *op, int *device, int *n_aggs, uint32_t *f64_mask, uint32_t *form_mask, int8_t *ident) {
  if (!op) return HSG_E_INVALID;
  *device = op->eng->device;
  *n_aggs = op->prog.n_out;
  uint32_t m = 0, fm = 0;
  for (int j = 0; j < op->prog.n_out; ++j) {
    if (op->prog.out_kind[j] != O_I64) m |= 1u << j;
    if (op->prog.form_kind[j] != F_NONE) fm |= 1u << j;
    // the reference's initial values: SUM Number 0, MIN maxBound, MAX minBound
    // (Codegen.hs:425-469); -1: an aggregate whose f64 prints exactly
    const int32_t kd = op->aggs[j].kind;
    ident[j] = kd == HSG_MIN ? 1 : kd == HSG_MAX ? 2 : kd == HSG_SUM ? 0 : -1;
  }
  *f64_mask = m;
  *form_mask = fm;
  return HSG_OK;
}
}  // namespace hsg

namespace hsg {
// For the sink encoder (sink.cpp): a select op's source records carry no key.
bool op_is_select(const hsg_op *op) { return op && op->select; }
}  // namespace hsg

namespace hsg {
// For the join (join.cpp): the engine's device.
int engine_device(const hsg_engine *e) { return e ? e->device : 0; }
int engine_nranks(const hsg_engine *e) { return e ? e->nranks : 1; }
int engine_split_comm(hsg_engine *e, Comm **out, int *rank, int *nranks, std::string &err) {
  *out = nullptr;
  *rank = e ? e->rank : 0;
  *nranks = e ? e->nranks : 1;
  if (!e || e->nranks <= 1 || !e->comm) {
    *rank = 0;
    *nranks = 1;
    return HSG_OK;
  }
  std::lock_guard<std::mutex> lk(e->mu);
  return comm_split(e->comm, out, err);
}
}  // namespace hsg
