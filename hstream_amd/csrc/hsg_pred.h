// The predicate interpreter of the WHERE / HAVING programs (include/
// hstream_gpu.h hsg_where_ins), device side: the operand stack, the exact
// i64 / f64 ordering and the instruction loop. k_where.hip runs it over a
// staged batch's value columns, k_having.hip over a changelog segment's
// aggregate columns, and k_map.hip runs its value half (value_step) to
// compute the derived columns; the semantics are written once, here.
//
// The program arrives as a kernel argument, so opcodes, column numbers and the
// value types (static: column type or constant kind) live in scalar registers
// and every branch over them is uniform across the wave. The operand stack is
// eight named entries shifted on push / pop -- constant indices only, so it
// stays in vector registers (no scratch) -- and the three-valued logic is a
// per-lane error bit beside each entry.
#pragma once

#include "hsg_where.h"

namespace hsg {
namespace pred {

constexpr int D = HSG_WHERE_MAX_DEPTH;

// The operand stack: v[0] is the top. Values are i64 or f64 bits, bools 0 / 1.
// err: bit k = entry k is the error value (per lane); f: bit k = entry k is
// f64 (uniform: derived from the program alone); form: bit k = entry k's
// literal-form bit (per lane; only the map pass reads it).
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

// The value half of the instruction set -- COL, I64, F64, ADD, SUB, MUL -- on
// the stack: cv[c] is the 8-byte word of column c (read for the columns the
// program names only), bit c of `absent` says the column is the error value
// for this row, bit c of `cform` is its literal-form bit, bit c of `f64` its
// type. False: `in` is none of these (the stack is untouched).
template <int NC>
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
  } else {
    return false;
  }
  return true;
}

// One row through the program (cv, absent: value_step). True = the row is
// kept (the result is true, not false and not the error).
template <int NC>
__device__ __forceinline__ bool eval(const WhereProg &p, const uint64_t (&cv)[NC], uint32_t absent) {
  Stack st;
  st.clear();
  for (int pc = 0; pc < p.n; ++pc) {
    const int32_t op = p.ins[pc].op;
    if (value_step(st, p.ins[pc], p.f64, cv, absent, 0u)) {
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
