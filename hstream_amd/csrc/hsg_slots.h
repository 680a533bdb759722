// The aggregate-slot algebra: what a record contributes to a slot, how two
// partial rows combine and the identity. Included by hsg_dev.h. Not part of
// the ABI. A few kernels keep a local form of one of these routines for their
// register budget (prec_elem, elems_v / combine_v / identity_v, sql_elems,
// ss_vw_elem, acc_row); each says so where it is defined, and a change to the
// slot set has to visit them too.
//
// Two small interfaces keep the rules independent of how a kernel holds its data:
//
//   program view PV   n(), op(s), col(s), and the free functions pv_aux(pv, s),
//                     pv_ties(pv), pv_last_form(pv, s). ProgRT reads the runtime
//                     Program, ProgSig<SIG> has the program baked into the
//                     kernel, ProgLds (hsg_sql.h) reads a copy in LDS. The
//                     routines here also take a Program itself (pv_n, pv_op,
//                     pv_col below).
//   record view R     present(c)  column c's field is there
//                     col(c)      its 8 bytes (an i64, or the bits of an f64)
//                     seq1()      the record's global sequence + 1 (0: the
//                                 program has no slot that reads it)
//                     dec(c)      column c's JSON literal is decimal
//                     A view may hold its words in an array, named registers,
//                     memory or LDS; the accessors are all rec_elems reads.
#pragma once

#include <initializer_list>
#include <type_traits>

#include "hsg_internal.h"

namespace hsg {

// ---------------------------------------------------------------------------
// Slot-program views
// ---------------------------------------------------------------------------
// The per-record LDS update dispatches on every slot's op. Read from the
// runtime Program (ProgRT) that dispatch is a scalar branch chain per slot and
// record; a program signature baked into the kernel (ProgSig<SIG>) folds it
// to the slot's one LDS atomic. SIG packs 7 bits per slot, slot 0 lowest:
// (op + 1) in the low 4 bits, the column in the high 3; 0 ends the program.
struct ProgRT {
  const Program &p;
  __device__ explicit ProgRT(const Program &q) : p(q) {}
  __device__ int n() const { return p.n_slots; }
  __device__ int op(int s) const { return p.slot_op[s]; }
  __device__ int col(int s) const { return p.slot_col[s]; }
};

template <uint64_t SIG, uint64_t SIG2 = 0>
struct ProgSig {
  // slot s's 7-bit code: slots 0..8 in SIG, 9..17 in SIG2 (programs of more
  // than 9 slots: the SQL drop-in's shape, literal forms and a passthrough)
  static constexpr uint32_t code(int s) {
    return s < 9 ? (uint32_t)((SIG >> (7 * s)) & 127u) : (uint32_t)((SIG2 >> (7 * (s - 9))) & 127u);
  }
  static constexpr int count() {
    int k = 0;
    while (k < 18 && (code(k) & 15u) != 0) ++k;
    return k;
  }
  static constexpr int op_of(int s) { return (int)(code(s) & 15u) - 1; }
  static constexpr int col_of(int s) { return (int)((code(s) >> 4) & 7u); }
  // the MIN / MAX slot a tie-word slot breaks ties of (build_program: the
  // one MIN (MAX) slot over the same column)
  static constexpr int aux_of(int s) {
    const int want = op_of(s) == S_TIE_MIN ? 0 : 1;
    for (int k = 0; k < count(); ++k) {
      const int o = op_of(k);
      const bool mn = o == S_MIN_I || o == S_MIN_F, mx = o == S_MAX_I || o == S_MAX_F;
      if (((want == 0 && mn) || (want == 1 && mx)) && col_of(k) == col_of(s)) return k;
    }
    return 0;
  }
  // the LAST_FORM slot over the column of LAST_SEQ slot s (-1: none): its
  // word is (seq + 1) << 1 | bit over the same present records, so the
  // LAST_SEQ slot is that word >> 1 and needs no update of its own
  static constexpr int last_form_of(int s) {
    for (int k = 0; k < count(); ++k)
      if (op_of(k) == S_LAST_FORM && col_of(k) == col_of(s)) return k;
    return -1;
  }
  static constexpr bool has_ties() {
    for (int k = 0; k < count(); ++k)
      if (op_of(k) == S_TIE_MIN || op_of(k) == S_TIE_MAX) return true;
    return false;
  }
  // a LAST pair or a literal-form slot: the slots that read seq1() / dec()
  static constexpr bool has_last_or_forms() {
    for (int k = 0; k < count(); ++k)
      if (op_of(k) == S_LAST_SEQ || op_of(k) == S_LAST_VAL || slot_is_form(op_of(k))) return true;
    return false;
  }
  __device__ ProgSig() {}
  __device__ explicit ProgSig(const Program &) {}
  __device__ constexpr int n() const { return count(); }
  __device__ constexpr int op(int s) const { return op_of(s); }
  __device__ constexpr int col(int s) const { return col_of(s); }
};

template <uint64_t SIG, uint64_t SIG2 = 0>
using ProgView = typename std::conditional<SIG == 0, ProgRT, ProgSig<SIG, SIG2>>::type;

// tie-word helpers over either view
__device__ inline int pv_aux(const ProgRT &pv, int s) { return pv.p.slot_aux[s]; }
__device__ inline bool pv_ties(const ProgRT &pv) { return pv.p.ties != 0; }
template <uint64_t SIG, uint64_t SIG2>
__device__ constexpr int pv_aux(const ProgSig<SIG, SIG2> &, int s) { return ProgSig<SIG, SIG2>::aux_of(s); }
template <uint64_t SIG, uint64_t SIG2>
__device__ constexpr bool pv_ties(const ProgSig<SIG, SIG2> &) { return ProgSig<SIG, SIG2>::has_ties(); }
__device__ inline int pv_last_form(const ProgRT &, int) { return -1; }
template <uint64_t SIG, uint64_t SIG2>
__device__ constexpr int pv_last_form(const ProgSig<SIG, SIG2> &, int s) { return ProgSig<SIG, SIG2>::last_form_of(s); }

// The routines below read a view through these, so that a Program is a view
// as it stands: wrapped as ProgRT the same slot loops compile to other code
// (they unroll where these stay rolled), and the sort-based per-record
// kernels k_seg_apply / k_seg_reduce of 8 and more slots lose occupancy.
// Which to use where: a runtime program is given to these routines as the
// Program (combine_row / combine_row_u are today instantiated over nothing
// else). ProgRT is the kernels' own runtime view (ProgView<0>, for their slot
// loops); it reaches rec_elems / identity_row at one place, RunsLds::aggs of
// k_ss_merge_big, which is templated on the view. ProgSig reaches rec_elems
// in k_agg_lean and the same place of k_ss_apply.
template <class PV>
__device__ inline int pv_n(const PV &pv) { return pv.n(); }
template <class PV>
__device__ inline int pv_op(const PV &pv, int s) { return pv.op(s); }
template <class PV>
__device__ inline int pv_col(const PV &pv, int s) { return pv.col(s); }
__device__ inline int pv_n(const Program &p) { return p.n_slots; }
__device__ inline int pv_op(const Program &p, int s) { return p.slot_op[s]; }
__device__ inline int pv_col(const Program &p, int s) { return p.slot_col[s]; }
__device__ inline int pv_aux(const Program &p, int s) { return p.slot_aux[s]; }
__device__ inline bool pv_ties(const Program &p) { return p.ties != 0; }

// signature of a runtime program (0: not expressible); slots past the ninth
// go to *sig2 when it is given (else such a program has no signature)
inline uint64_t program_sig(const Program &p, uint64_t *sig2 = nullptr) {
  if (p.n_slots > (sig2 ? 18 : 8)) return 0;
  uint64_t sig = 0, hi = 0;
  for (int s = 0; s < p.n_slots; ++s) {
    if (p.slot_op[s] < 0 || p.slot_op[s] > 14 || p.slot_col[s] < 0 || p.slot_col[s] > 7) return 0;
    // (a tie word's MIN / MAX slot is implied: the one over its column)
    if (slot_is_tie(p.slot_op[s])) {
      const int v = p.slot_aux[s], vo = p.slot_op[v];
      const bool ok = p.slot_col[v] == p.slot_col[s] &&
                      (p.slot_op[s] == S_TIE_MIN ? (vo == S_MIN_I || vo == S_MIN_F) : (vo == S_MAX_I || vo == S_MAX_F));
      if (!ok) return 0;
    }
    const uint64_t c = (uint64_t)((p.slot_op[s] + 1) | (p.slot_col[s] << 4));
    if (s < 9) sig |= c << (7 * s);
    else hi |= c << (7 * (s - 9));
  }
  if (sig2) *sig2 = hi;
  return sig;
}

// signature of a one-column program from its ops; sig_ops_at: the nine slots
// from `first` on (the second word of a program of more than nine slots)
constexpr uint64_t sig_ops(std::initializer_list<int> ops) {
  uint64_t sig = 0;
  int k = 0;
  for (int op : ops) sig |= (uint64_t)(op + 1) << (7 * k++);
  return sig;
}
constexpr uint64_t sig_ops_at(std::initializer_list<int> ops, int first) {
  uint64_t sig = 0;
  int k = 0;
  for (int op : ops) {
    if (k >= first && k < first + 9) sig |= (uint64_t)(op + 1) << (7 * (k - first));
    ++k;
  }
  return sig;
}

// ---------------------------------------------------------------------------
// Identity
// ---------------------------------------------------------------------------
__device__ inline int64_t slot_identity_dev(int32_t op) {
  switch (op) {
    case S_MIN_I: return INT64_MAX;
    case S_MAX_I: return INT64_MIN;
    case S_MIN_F: return (int64_t)f64_ord(9223372036854775807.0);
    case S_MAX_F: return (int64_t)f64_ord(-9223372036854775808.0);
    case S_SUM_F: return INT64_MIN;  // -0.0 (slot_identity)
    case S_TIE_MIN: return 1;        // seq 0, integral: the initial maxBound
    default: return 0;
  }
}

// Element of a present f64 for a MIN / MAX slot of a group that starts from
// its first record's element instead of an identity row (the session merge
// path's point sessions): the fold's initial value maxBound / minBound
// (Codegen.hs:438,451) lies inside the f64 range, and a value beyond it never
// replaces it. Not for ops with tie words (there the bound has a word of its own).
__device__ inline int64_t f64_extreme_elem(int op, double d) {
  const uint64_t o = f64_ord(d), id = (uint64_t)slot_identity_dev(op);
  return (int64_t)(op == S_MIN_F ? (o < id ? o : id) : (o > id ? o : id));
}

// ---------------------------------------------------------------------------
// Record -> slot element
// ---------------------------------------------------------------------------
// Contribution of record r to slot s: the state of a group holding only r
// (the identity when the field is absent; a LAST_VAL slot, read only beside
// its LAST_SEQ, holds 0 then).
template <class PV, class R>
__device__ inline int64_t rec_elem(const PV &pv, int s, const R &r) {
  const int op = pv_op(pv, s), c = pv_col(pv, s);
  if (op == S_CNT_ALL) return 1;
  if (op == S_LAST_VAL) return r.present(c) ? r.col(c) : 0;
  if (!r.present(c)) return slot_identity_dev(op);
  switch (op) {
    case S_CNT: return 1;
    case S_MIN_F:
    case S_MAX_F: return (int64_t)f64_ord(__builtin_bit_cast(double, r.col(c)));
    case S_LAST_SEQ: return (int64_t)r.seq1();
    case S_CNT_DEC: return r.dec(c) ? 1 : 0;
    case S_TIE_MIN:
    case S_TIE_MAX:
    case S_LAST_FORM: return (int64_t)(((uint64_t)r.seq1() << 1) | (r.dec(c) ? 0u : 1u));
    case S_SUM_I:
    case S_SUM_F:
    case S_MIN_I:
    case S_MAX_I: return r.col(c);
    default: return 0;
  }
}
// (always inlined: outlined, the row it fills would live in scratch)
template <int MS, class PV, class R>
__device__ __attribute__((always_inline)) inline void rec_elems(const PV &pv, const R &r, int64_t (&e)[MS]) {
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    e[s] = 0;
    if (s < pv_n(pv)) e[s] = rec_elem(pv, s, r);
  }
}

__device__ inline bool rec_present(const Batch &b, int c, uint64_t i) {
  return b.valid[c] == nullptr || b.valid[c][i] != 0;
}
// the value's JSON literal prints in Generic form (bit 1 of its valid byte,
// hstream_ingest.h literal_forms)
__device__ inline bool rec_decimal(const Batch &b, int c, uint64_t i) {
  return b.valid[c] != nullptr && (b.valid[c][i] & 2u) != 0;
}
// record i of a batch's columns
struct BatchRec {
  const Batch &b;
  uint64_t i, seq;
  __device__ bool present(int c) const { return rec_present(b, c, i); }
  __device__ int64_t col(int c) const { return b.col[c][i]; }
  __device__ uint64_t seq1() const { return seq; }
  __device__ bool dec(int c) const { return rec_decimal(b, c, i); }
};

// A session-partitioned record over its raw words: word 0 = key | present
// bits << 32, ts, column c at w[2 + c]. DEC: bit of word 0 with column 0's
// decimal-literal flag (40 in the bucket replay's records), 0 = the records
// carry none and dec() is false. The merge path builds its records without
// flags or sequence numbers (seq1 = 0): the host admits it only for programs
// without LAST and literal-form slots (session.cpp, ss_merge), the only
// slots that would read them.
template <int DEC = 0>
struct SessRec {
  const uint64_t *w;
  uint64_t hi, seq;  // word 0's high half
  __device__ SessRec(const uint64_t *rec, uint64_t seq1 = 0) : w(rec), hi(rec[0] >> 32), seq(seq1) {}
  __device__ bool present(int c) const { return (hi >> c) & 1ull; }
  __device__ int64_t col(int c) const { return (int64_t)w[2 + c]; }
  __device__ uint64_t seq1() const { return seq; }
  __device__ bool dec(int c) const { return DEC != 0 && ((hi >> (DEC - 32 + c)) & 1ull); }
};

// ---------------------------------------------------------------------------
// Combine
// ---------------------------------------------------------------------------
// a <- a (+) e for one slot, where e comes later in arrival order than a.
// LAST_SEQ/LAST_VAL are combined as a pair by the caller (see combine_row).
__device__ inline int64_t slot_combine(int op, int64_t a, int64_t e) {
  switch (op) {
    case S_CNT_ALL:
    case S_CNT:
    case S_SUM_I: return (int64_t)((uint64_t)a + (uint64_t)e);
    case S_SUM_F: return __builtin_bit_cast(int64_t, __builtin_bit_cast(double, a) + __builtin_bit_cast(double, e));
    case S_MIN_I: return e < a ? e : a;
    case S_MAX_I: return e > a ? e : a;
    case S_MIN_F: return (uint64_t)e < (uint64_t)a ? e : a;
    case S_MAX_F: return (uint64_t)e > (uint64_t)a ? e : a;
    case S_CNT_DEC: return (int64_t)((uint64_t)a + (uint64_t)e);
    case S_LAST_FORM: return (uint64_t)e > (uint64_t)a ? e : a;
    default: return a;  // S_TIE_*: combined with their MIN / MAX slot (tie_combine)
  }
}

// "e is better than a" for the MIN / MAX slot op vop (equal: a tie)
__device__ inline bool extreme_better(int vop, int64_t e, int64_t a) {
  switch (vop) {
    case S_MIN_I: return e < a;
    case S_MAX_I: return e > a;
    case S_MIN_F: return (uint64_t)e < (uint64_t)a;
    case S_MAX_F: return (uint64_t)e > (uint64_t)a;
    default: return false;
  }
}
// tie word after a <- a (+) e, from the MIN / MAX values before the combine
// (va, ve): the better value's word; on a tie the earlier literal for MIN
// (min n x = n) and the later for MAX (max n x = x) -- by record sequence, so
// any grouping of a record fold gives the sequential fold's word
__device__ inline int64_t tie_combine(int op, int vop, int64_t va, int64_t ve, int64_t ta, int64_t te) {
  if (extreme_better(vop, ve, va)) return te;
  if (va != ve) return ta;
  if (op == S_TIE_MIN) return (uint64_t)te < (uint64_t)ta ? te : ta;
  return (uint64_t)te > (uint64_t)ta ? te : ta;
}

// Row-wise combine over MS compile-time-bounded slots (registers, no scratch).
// the value of slot v of a register row (v not a compile-time index)
template <int MS>
__device__ inline int64_t reg_at(const int64_t (&r)[MS], int v) {
  int64_t x = 0;
#pragma unroll
  for (int s = 0; s < MS; ++s)
    if (s == v) x = r[s];
  return x;
}

// Slot s's step of a <- a (+) e. TIES: the pass over the tie words, which runs
// first, against the MIN / MAX values before the combine; then the pass over
// every other slot, the LAST pair taken together.
template <bool TIES, int MS, class PV>
__device__ inline void combine_slot(const PV &pv, int s, int64_t (&a)[MS], const int64_t (&e)[MS]) {
  const int op = pv_op(pv, s);
  if constexpr (TIES) {
    if (!slot_is_tie(op)) return;
    const int v = pv_aux(pv, s);
    a[s] = tie_combine(op, pv_op(pv, v), reg_at<MS>(a, v), reg_at<MS>(e, v), a[s], e[s]);
  } else if (op == S_LAST_SEQ) {
    if (e[s] != 0) {
      a[s] = e[s];
      if (s + 1 < MS) a[s + 1] = e[s + 1];
    }
  } else if (op != S_LAST_VAL) {
    a[s] = slot_combine(op, a[s], e[s]);
  }
}
template <bool TIES, int MS, class PV>
__device__ inline void combine_pass(const PV &pv, int64_t (&a)[MS], const int64_t (&e)[MS]) {
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    if (s >= pv_n(pv)) break;
    combine_slot<TIES, MS>(pv, s, a, e);
  }
}
template <int MS, class PV>
__device__ inline void combine_row(const PV &pv, int64_t (&a)[MS], const int64_t (&e)[MS]) {
  if (pv_ties(pv)) combine_pass<true, MS>(pv, a, e);
  combine_pass<false, MS>(pv, a, e);
}

// The same with the slot loops unrolled by the front end (S: the recursion's
// slot), for the 24-slot class of k_sql_apply: there the optimizer leaves the
// loops above rolled, which puts the rows they index in scratch.
template <bool TIES, int MS, int S = 0, class PV>
__device__ inline void combine_pass_u(const PV &pv, int64_t (&a)[MS], const int64_t (&e)[MS]) {
  if constexpr (S < MS) {
    if (S < pv_n(pv)) combine_slot<TIES, MS>(pv, S, a, e);
    combine_pass_u<TIES, MS, S + 1>(pv, a, e);
  }
}
template <int MS, class PV>
__device__ inline void combine_row_u(const PV &pv, int64_t (&a)[MS], const int64_t (&e)[MS]) {
  if (pv_ties(pv)) combine_pass_u<true, MS>(pv, a, e);
  combine_pass_u<false, MS>(pv, a, e);
}

template <int MS, class PV>
__device__ inline void identity_row(const PV &pv, int64_t (&a)[MS]) {
#pragma unroll
  for (int s = 0; s < MS; ++s) a[s] = s < pv_n(pv) ? slot_identity_dev(pv_op(pv, s)) : 0;
}

// Session merge, acc <- sessionMergeF rk acc cur (SessionWindowedStream.hs
// :100-114; acc = the new record with the sessions merged so far, cur = the
// next overlapped session in end order): the aggregate components'
// aggregateMergeF (Codegen.hs:409-469) -- counts and sums add, MIN / MAX keep
// the extreme with min n1 n2 / max n1 n2 on ties (n1 = acc's literal for
// MIN, n2 = cur's for MAX), passthrough columns take cur's (o2)
template <int MS>
__device__ inline void merge_row(const Program &prog, int64_t (&acc)[MS], const int64_t (&cur)[MS]) {
  if (prog.ties) {
#pragma unroll
    for (int s = 0; s < MS; ++s) {
      if (s >= prog.n_slots) break;
      const int op = prog.slot_op[s];
      if (!slot_is_tie(op)) continue;
      const int v = prog.slot_aux[s], vop = prog.slot_op[v];
      const int64_t va = reg_at<MS>(acc, v), vc = reg_at<MS>(cur, v);
      if (extreme_better(vop, vc, va) || (va == vc && op == S_TIE_MAX)) acc[s] = cur[s];
    }
  }
#pragma unroll
  for (int s = 0; s < MS; ++s) {
    if (s >= prog.n_slots) break;
    const int op = prog.slot_op[s];
    if (op == S_LAST_SEQ || op == S_LAST_VAL || op == S_LAST_FORM) acc[s] = cur[s];
    else acc[s] = slot_combine(op, acc[s], cur[s]);
  }
}

}  // namespace hsg
