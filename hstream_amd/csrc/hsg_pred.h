// The interpreter of the row programs (include/hstream_gpu.h hsg_where_ins),
// device side: a record's named columns, the operand stack, the exact i64 /
// f64 ordering, the instruction loop of a predicate and the runs of a map's
// value programs. Every pass that runs a program per row goes through here;
// the semantics are written once.
//
// The program arrives as a kernel argument, so opcodes, column numbers and the
// value types (static: column type or constant kind) live in scalar registers
// and every branch over them is uniform across the wave. The operand stack is
// eight named entries shifted on push / pop -- constant indices only, so it
// stays in vector registers (no scratch) -- and the three-valued logic is a
// per-lane error bit beside each entry.
//
// Everything that interprets is templated on the kernel's function class FC
// (hsg_where.h prog_fn_class): 0 has no HSG_W_FN branch, 1 the exact family, 2
// all 22 functions. Each kernel is instantiated per class and the host
// launches the class of the op's program, because a branch of the interpreter
// costs its registers whether or not it is taken.
#pragma once

#include "hsg_where.h"

namespace hsg {
namespace pred {

constexpr int D = HSG_WHERE_MAX_DEPTH;

// The operand stack: v[0] is the top. Values are i64 or f64 bits, bools 0 / 1.
// err: bit k = entry k is the error value (per lane); f: bit k = entry k is
// f64 (uniform: derived from the program alone); form: bit k = entry k's
// literal-form bit (per lane; only run_exprs hands it on).
struct Stack {
  uint64_t v[D];
  uint32_t err;
  uint32_t f;
  uint32_t form;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] = 0;
    err = 0;
    f = 0;
    form = 0;
  }
  __device__ __forceinline__ void push(uint64_t x, bool e, bool isf, bool fm = false) {
#pragma unroll
    for (int k = D - 1; k > 0; --k) v[k] = v[k - 1];
    v[0] = x;
    err = (err << 1) | (e ? 1u : 0u);
    f = (f << 1) | (isf ? 1u : 0u);
    form = (form << 1) | (fm ? 1u : 0u);
  }
  __device__ __forceinline__ void pop() {
#pragma unroll
    for (int k = 0; k < D - 1; ++k) v[k] = v[k + 1];
    err >>= 1;
    f >>= 1;
    form >>= 1;
  }
};

__device__ __forceinline__ double as_f64(uint64_t u) { return __builtin_bit_cast(double, u); }
__device__ __forceinline__ uint64_t as_u64(double d) { return __builtin_bit_cast(uint64_t, d); }

// Record i's named columns: cv[c] is the 8-byte word of each column `cols`
// names (0 for the others, and for every column when the lane is past the
// batch: !in), every load in flight before the first use. The valid-byte rule
// lives here: bit 0 alone says present -- bit c of `absent` is its complement
// -- bit 1 is the literal form -- bit c of `cform`, 0 unless `forms` -- and a
// null valid array is all present. A pass that keeps no forms passes forms = 0
// and drops cform.
__device__ __forceinline__ void load_cols(uint32_t cols, const int64_t *const (&col)[kMaxCols],
                                          const uint8_t *const (&valid)[kMaxCols], uint64_t i, bool in, uint32_t forms,
                                          uint64_t (&cv)[kMaxCols], uint32_t &absent, uint32_t &cform) {
  uint32_t vb[kMaxCols];
#pragma unroll
  for (int c = 0; c < kMaxCols; ++c) {
    cv[c] = 0;
    vb[c] = 1;
    if ((cols >> c) & 1u) {
      if (in) cv[c] = (uint64_t)col[c][i];
      if (in && valid[c]) vb[c] = valid[c][i];
    }
  }
  absent = 0;
  cform = 0;
#pragma unroll
  for (int c = 0; c < kMaxCols; ++c) {
    absent |= ((vb[c] & 1u) ^ 1u) << c;
    cform |= ((vb[c] >> 1) & 1u) << c;
  }
  if (!forms) cform = 0;
}

// Bit c: word c is an f64 (bit c of `f64cols`) that is NaN. Ahead of a HAVING
// program that is the error value: an aggregate or an expression that has no
// number (AVG of no value) is stored as NaN.
template <int NC>
__device__ __forceinline__ uint32_t nan_mask(const uint64_t (&w)[NC], uint32_t f64cols) {
  uint32_t m = 0;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const double d = as_f64(w[c]);
    if ((f64cols >> c) & 1u) m |= d != d ? 1u << c : 0u;
  }
  return m;
}

// Ordering of two values as Scientific orders them: -1 / 0 / 1, 2 = unordered
// (a NaN, which no JSON number is). An i64 against an f64 is compared exactly:
// the integer is never rounded to a double (2^53 + 1 > 9007199254740992.0,
// INT64_MAX < 2^63).
__device__ __forceinline__ int cmp_i_f(int64_t i, double d) {
  if (d != d) return 2;
  if (d >= 9223372036854775808.0) return -1;
  if (d < -9223372036854775808.0) return 1;
  const double t = __builtin_trunc(d);  // |t| <= 2^63, exact as an i64 unless t = -2^63 (also exact)
  const int64_t ti = (int64_t)t;
  if (i != ti) return i < ti ? -1 : 1;
  return d > t ? -1 : (d < t ? 1 : 0);
}
__device__ __forceinline__ int cmp_vals(uint64_t a, bool af, uint64_t b, bool bf) {
  if (!af && !bf) return (int64_t)a < (int64_t)b ? -1 : ((int64_t)a > (int64_t)b ? 1 : 0);
  if (af && bf) {
    const double x = as_f64(a), y = as_f64(b);
    return x < y ? -1 : (x > y ? 1 : (x == y ? 0 : 2));
  }
  if (!af) return cmp_i_f((int64_t)a, as_f64(b));
  const int c = cmp_i_f((int64_t)b, as_f64(a));
  return c == 2 ? 2 : -c;
}

// HSG_W_FN on the top of the stack: the numeric function `fn` (hsg_fn, uniform
// like the opcode), include/hstream_gpu.h and DESIGN.md 9 for the rules. FC is
// the kernel's function class: 1 holds the exact family (ABS, CEIL, FLOOR,
// ROUND, SIGN, SQRT), 2 all 22; the host launches the class of the op's
// programs, so a class-1 kernel never meets another function. Every f64 result
// passes through `+ 0.0`: a Scientific has no negative zero.
template <int FC>
__device__ __forceinline__ void fn_step(Stack &st, int32_t fn) {
  const uint64_t x = st.v[0];
  const bool xf = st.f & 1u;
  const double xd = xf ? as_f64(x) : (double)(int64_t)x;  // toRealFloat
  // the error value: the operand is, or it is an f64 that is not finite
  bool e = (st.err & 1u) || (xf && !(xd - xd == 0.0));
  bool fm = st.form & 1u;
  bool of = xf;
  uint64_t o = x;
  if (fn == HSG_FN_ABS) {
    // (the form bit stays: abs keeps a Scientific's exponent)
    o = xf ? as_u64(__builtin_fabs(xd)) : ((int64_t)x < 0 ? 0ull - x : x);
  } else if (fn == HSG_FN_CEIL || fn == HSG_FN_FLOOR || fn == HSG_FN_ROUND) {
    // an i64 is its own ceiling; an f64 stays an f64 (exact for every double)
    if (xf) {
      const double r = fn == HSG_FN_CEIL ? __builtin_ceil(xd) : (fn == HSG_FN_FLOOR ? __builtin_floor(xd) : __builtin_rint(xd));
      o = as_u64(r + 0.0);
    }
    fm = false;
  } else if (fn == HSG_FN_SIGN) {
    const bool pos = xf ? xd > 0.0 : (int64_t)x > 0, neg = xf ? xd < 0.0 : (int64_t)x < 0;
    o = (uint64_t)((int64_t)pos - (int64_t)neg);
    of = false;
    fm = false;
  } else {
    // the f64 functions. The domain tests read the converted operand: (double)
    // is monotonic and exact at -1, 0 and 1, so an i64 tests as the integer it is
    double r = 0.0;
    bool dom = false;
    if (fn == HSG_FN_SQRT) {
      dom = xd < 0.0;
      r = ::sqrt(xd);
    }
    if constexpr (FC >= 2) {
      switch (fn) {
        case HSG_FN_SIN: r = ::sin(xd); break;
        case HSG_FN_SINH: r = ::sinh(xd); break;
        case HSG_FN_ASIN: dom = xd < -1.0 || xd > 1.0; r = ::asin(xd); break;
        case HSG_FN_ASINH: r = ::asinh(xd); break;
        case HSG_FN_COS: r = ::cos(xd); break;
        case HSG_FN_COSH: r = ::cosh(xd); break;
        case HSG_FN_ACOS: dom = xd < -1.0 || xd > 1.0; r = ::acos(xd); break;
        case HSG_FN_ACOSH: dom = xd < 1.0; r = ::acosh(xd); break;
        case HSG_FN_TAN: r = ::tan(xd); break;
        case HSG_FN_TANH: r = ::tanh(xd); break;
        case HSG_FN_ATAN: r = ::atan(xd); break;
        case HSG_FN_ATANH: dom = xd <= -1.0 || xd >= 1.0; r = ::atanh(xd); break;
        // LOG2 / LOG10 as the reference divides (Internal/Codegen.hs:173-178): the doubles log(2.0), log(10.0)
        case HSG_FN_LOG: dom = xd <= 0.0; r = ::log(xd); break;
        case HSG_FN_LOG2: dom = xd <= 0.0; r = ::log(xd) / 0.6931471805599453; break;
        case HSG_FN_LOG10: dom = xd <= 0.0; r = ::log(xd) / 2.302585092994046; break;
        case HSG_FN_EXP: r = ::exp(xd); break;
        default: break;
      }
    }
    r += 0.0;
    e = e || dom || !(r - r == 0.0);
    o = as_u64(r);
    of = true;
    fm = r != __builtin_trunc(r);  // fromFloatDigits of an integral double has no negative exponent
  }
  st.pop();
  st.push(o, e, of, fm);
}

// The value half of the instruction set -- COL, I64, F64, ADD, SUB, MUL, and in
// a kernel of function class FC > 0 also FN -- on the stack: cv[c] is the
// 8-byte word of column c (read for the columns the program names only), bit
// c of `absent` says the column is the error value for this row, bit c of
// `cform` is its literal-form bit, bit c of `f64` its type. False: `in` is
// none of these (the stack is untouched). FC = 0 has no FN branch at all: a
// branch costs its registers taken or not.
template <int FC, int NC>
__device__ __forceinline__ bool value_step(Stack &st, const hsg_where_ins &in, uint32_t f64, const uint64_t (&cv)[NC],
                                           uint32_t absent, uint32_t cform) {
  const int32_t op = in.op;
  if (op == HSG_W_COL) {
    const int32_t c = in.arg;
    uint64_t x = 0;
#pragma unroll
    for (int k = 0; k < NC; ++k) x = c == k ? cv[k] : x;
    st.push(x, (absent >> c) & 1u, (f64 >> c) & 1u, (cform >> c) & 1u);
  } else if (op == HSG_W_I64 || op == HSG_W_F64) {
    // (a map's constants carry their literal-form bit in `arg`)
    st.push((uint64_t)in.imm.i, false, op == HSG_W_F64, in.arg & 1);
  } else if (op <= HSG_W_MUL) {
    // value value -> value: i64 wraps, anything with an f64 is f64
    const uint64_t r = st.v[0], l = st.v[1];
    const bool rf = st.f & 1u, lf = (st.f >> 1) & 1u;
    const bool e = (st.err & 3u) != 0;
    const bool fm = (st.form & 3u) != 0;
    uint64_t o;
    if (!lf && !rf) {
      o = op == HSG_W_ADD ? l + r : (op == HSG_W_SUB ? l - r : l * r);
    } else {
      const double x = lf ? as_f64(l) : (double)(int64_t)l, y = rf ? as_f64(r) : (double)(int64_t)r;
      o = as_u64(op == HSG_W_ADD ? x + y : (op == HSG_W_SUB ? x - y : x * y));
    }
    st.pop();
    st.pop();
    st.push(o, e, lf || rf, fm);
  } else if (FC > 0 && op == HSG_W_FN) {
    if constexpr (FC > 0) fn_step<FC>(st, in.arg);
  } else {
    return false;
  }
  return true;
}

// A map's value programs over one row (cv, absent, cform: load_cols), one run
// after the other on one stack: run r is ins[end[r - 1] .. end[r]) and leaves
// one value, the top of the stack, which at_end(r, value, err, form) takes --
// err and form are 0 / 1, that value's error and derived literal-form bit.
template <int FC, class F>
__device__ __forceinline__ void run_exprs(const MapProg &p, const uint64_t (&cv)[kMaxCols], uint32_t absent,
                                          uint32_t cform, F &&at_end) {
  Stack st;
  st.clear();
  int r = 0;
  for (int pc = 0; pc < p.n_ins; ++pc) {
    value_step<FC>(st, p.ins[pc], p.f64, cv, absent, cform);
    if (pc + 1 == p.end[r]) {
      at_end(r, st.v[0], st.err & 1u, st.form & 1u);
      st.pop();
      ++r;
    }
  }
}

// One row through the program (cv, absent: value_step). True = the row is
// kept (the result is true, not false and not the error).
template <int FC, int NC>
__device__ __forceinline__ bool eval(const WhereProg &p, const uint64_t (&cv)[NC], uint32_t absent) {
  Stack st;
  st.clear();
  for (int pc = 0; pc < p.n; ++pc) {
    const int32_t op = p.ins[pc].op;
    if (value_step<FC>(st, p.ins[pc], p.f64, cv, absent, 0u)) {
    } else if (op <= HSG_W_GE) {
      // value value -> bool; error if either operand is
      const int c = cmp_vals(st.v[1], (st.f >> 1) & 1u, st.v[0], st.f & 1u);
      const bool e = (st.err & 3u) != 0;
      bool o;
      switch (op) {
        case HSG_W_EQ: o = c == 0; break;
        case HSG_W_NE: o = c != 0; break;
        case HSG_W_LT: o = c == -1; break;
        case HSG_W_GT: o = c == 1; break;
        case HSG_W_LE: o = c == -1 || c == 0; break;
        default: o = c == 1 || c == 0; break;
      }
      st.pop();
      st.pop();
      st.push(o ? 1 : 0, e, false);
    } else if (op == HSG_W_BETWEEN) {
      // lo x hi (Codegen.hs:331-341): lo > x decides before hi is looked at
      const int c1 = cmp_vals(st.v[2], (st.f >> 2) & 1u, st.v[1], (st.f >> 1) & 1u);
      const int c2 = cmp_vals(st.v[1], (st.f >> 1) & 1u, st.v[0], st.f & 1u);
      const bool e_lox = (st.err & 6u) != 0, e_hi = (st.err & 1u) != 0;
      const bool gt1 = c1 == 1;
      const bool e = e_lox || (!gt1 && e_hi);
      const bool o = !gt1 && c2 != 1 && c1 != 2 && c2 != 2;
      st.pop();
      st.pop();
      st.pop();
      st.push(o ? 1 : 0, e, false);
    } else if (op == HSG_W_NOT) {
      st.v[0] ^= 1ull;  // NOT(error) = error: the bit stays
    } else {
      // AND / OR over (l, r), both computed: l decides when it is false
      // (AND) / true (OR) or the error; else the result is r
      const bool l = st.v[1] != 0, r = st.v[0] != 0;
      const bool le = (st.err >> 1) & 1u, re = st.err & 1u;
      const bool take_l = le || (op == HSG_W_AND ? !l : l);
      const bool o = take_l ? l : r, e = take_l ? le : re;
      st.pop();
      st.pop();
      st.push(o ? 1 : 0, e, false);
    }
  }
  return st.v[0] != 0 && !(st.err & 1u);
}

}  // namespace pred
}  // namespace hsg
