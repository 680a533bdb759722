// Lean aggregation of the SQL drop-in's op shape: every windowed GROUP BY that
// genGroupByNode dispatches prints its values through objectSerde with their
// Scientific literal forms (HSG_OPF_LITERAL_FORMS: MIN / MAX fold with
// `min n x` / `max n x`, Codegen.hs:436-461) and keeps every non-aggregate
// SELECT column as a passthrough, the value of the group's last record
// (HSG_LAST, Codegen.hs:463-469). For packed one-window batches (tumbling,
// unwindowed), in two launches, as k_agg_lean.hip:
//
//   k_agg_sql    one workgroup per bucket chunk: the chunk's packed records
//                [header][column(s)][sequence word] (hsg_dev.h seq_word: the
//                record's global sequence + 1 and its decimal-literal bits)
//                into an LDS hash table, then the live groups as partials
//                [g][slot 0 .. n-1] (the op's full slot program, global
//                sequence words) in HBM-home order;
//   k_sql_apply  one workgroup per aggregation workgroup: its partials into
//                the HBM (key, window) table with the full slot algebra
//                (hsg_slots.h combine_row: tie words, the LAST pair, form
//                slots) and the per-batch changelog rows written directly.
//
// The order-dependent slots need more than one LDS atomic per slot. The
// chunk's records are taken in blocks of RB x NT, each in two phases:
//   1. atomics: counts, sums, MIN / MAX, the LAST sequence (max of seq + 1),
//      LAST_FORM (max of (seq + 1) << 1 | integral); a record that lowers a
//      MIN (raises a MAX) clears the slot's tie word -- the words of earlier
//      records belong to a value that is no longer extreme;
//   2. after a barrier, the extremes and last sequences of the block are
//      final: the record whose sequence is the group's LAST sequence writes
//      the LAST value (one writer: sequences are unique), and every record
//      whose value equals the group's MIN (MAX) folds its tie word in with an
//      atomic min (max): the earliest literal among the minima (`min n x = n`),
//      the latest among the maxima (`max n x = x`).
// A second barrier ends the block when the program has tie words (the next
// block's resets must not meet this block's tie atomics); without them a
// later block's LAST writer always writes after this block's (it passes the
// next barrier only once every thread has finished this phase). Records never
// need to arrive in order: the sequence numbers carry it.
//
// Every packed batch is finished exactly here. A chunk with more groups than
// its LDS table holds is taken in key-hash rounds (one partial per group
// still); when no finer split is left a record that finds no room becomes a
// partial of its own, and a bucket split over several workgroups gives
// several partials per group: k_sql_apply combines those under the row's
// lock, in any order. Only a batch that is not packed (late records, a wide
// layout) runs on the careful path (k_window.hip's record kernels).
//
// The kernels are in hsg_sql.h. This unit holds the variants for records of
// one or two columns and programs of at most 16 slots (k_agg_sql: whole
// records in registers) and the dispatch; k_agg_sql_wide.hip holds those for
// 3 - 8 columns and for 17 - 24 slots (k_agg_sql_wide).
#include "hsg_sql.h"

namespace hsg {

// LDS entries of the SQL lean kernel for this program (op_device.cpp
// adapt_partitions: buckets of at most half a table of groups); the 24-slot
// class keeps 512 (k_agg_sql_wide.hip)
uint64_t sql_lds_entries(const Program &prog) {
  if (prog.n_slots > 16) return 512;
  uint64_t hi = 0;
  const uint64_t sq = program_sig(prog, &hi);
  return ((sq == kSigSqlI && hi == kSigSqlI2) || (sq == kSigSqlF && hi == kSigSqlF2) || (sq == kSigSqlSumMaxI && !hi))
             ? 2048
             : 1024;
}

// the op shape this path takes: one-window packed records with the sequence
// word, the full slot program in LDS: one or two columns and <= 16 slots, or
// (pp.sql_wide: an op created for them) up to 8 columns and kMaxSlots slots
bool sql_lean_eligible(const Program &prog, const PartParams &pp) {
  if (pp.pane_S != 1 || !pp.has_seq) return false;
  if ((pp.words == 4 || pp.words == 5) && prog.n_slots <= 16) return true;
  return pp.sql_wide && pp.words >= 4 && pp.words <= kPartMaxWords && prog.n_slots <= kMaxSlots;
}

template <int MS, int E, int NT, uint64_t SIG = 0, uint64_t SIG2 = 0>
static void sql_launch(hipStream_t s, dim3 g, const Program &prog, const TwParams &p, const PartParams &pp,
                       const TwTable &t, const PartBuffers &pb, DevScalars *sc, const OutCols &out, uint64_t out_base,
                       uint64_t out_cap) {
  if (pp.words - 1 == 3)
    hipLaunchKernelGGL((k_agg_sql<MS, E, NT, 3, SIG, SIG2>), g, dim3(NT), 0, s, prog, pp, t, pb, sc);
  else
    hipLaunchKernelGGL((k_agg_sql<MS, E, NT, 4, SIG, SIG2>), g, dim3(NT), 0, s, prog, pp, t, pb, sc);
  hipLaunchKernelGGL((k_sql_apply<MS>), g, dim3(256), 0, s, prog, p, pp, t, pb, out, out_base, out_cap, sc);
}

bool launch_part_agg_sql(hipStream_t s, dim3 g, const Program &prog, const TwParams &p, const PartParams &pp,
                         const TwTable &t, const PartBuffers &pb, DevScalars *sc, const OutCols *out,
                         uint64_t out_base, uint64_t out_cap) {
  if (!sql_lean_eligible(prog, pp)) return false;
  OutCols oc;
  memset(&oc, 0, sizeof(oc));
  if (out) oc = *out;
  if (sql_wide_shape(prog, pp)) {
    // 3 - 8 columns or 17 - 24 slots: k_agg_sql_wide, then the apply of the
    // program's slot class
    launch_sql_wide_agg(s, g, prog, pp, t, pb, sc);
    if (prog.n_slots > 16)
      launch_sql_apply24(s, g, prog, p, pp, t, pb, oc, out_base, out_cap, sc);
    else if (prog.n_slots > 12)
      hipLaunchKernelGGL((k_sql_apply<16>), g, dim3(256), 0, s, prog, p, pp, t, pb, oc, out_base, out_cap, sc);
    else if (prog.n_slots > 8)
      hipLaunchKernelGGL((k_sql_apply<12>), g, dim3(256), 0, s, prog, p, pp, t, pb, oc, out_base, out_cap, sc);
    else
      hipLaunchKernelGGL((k_sql_apply<8>), g, dim3(256), 0, s, prog, p, pp, t, pb, oc, out_base, out_cap, sc);
    return true;
  }
  // 1024 LDS entries (part_lds_entries: buckets of <= 512 groups): 8 + 8 MS
  // bytes each, one 1024-thread workgroup per CU at 12 slots
  // the SQL drop-in's C2 and C5 queries: their slot programs baked in, in
  // the packed LDS layout (a 2048-entry table, buckets of twice the groups)
  uint64_t hi = 0;
  const uint64_t sq = program_sig(prog, &hi);
  if (prog.n_slots <= 8) {
    if (sq == kSigSqlSumMaxI && !hi)
      sql_launch<8, 2048, 1024, kSigSqlSumMaxI, 0>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
    else
      sql_launch<8, 1024, 512>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
  } else if (prog.n_slots <= 12) {
    if (sq == kSigSqlI && hi == kSigSqlI2)
      sql_launch<12, 2048, 1024, kSigSqlI, kSigSqlI2>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
    else if (sq == kSigSqlF && hi == kSigSqlF2)
      sql_launch<12, 2048, 1024, kSigSqlF, kSigSqlF2>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
    else
      sql_launch<12, 1024, 1024>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
  }
  else sql_launch<16, 1024, 1024>(s, g, prog, p, pp, t, pb, sc, oc, out_base, out_cap);
  return true;
}

}  // namespace hsg
