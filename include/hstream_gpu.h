/*
 * hstream_gpu.h — C ABI of libhstream_gpu, the MI355X (gfx950) engine behind
 * HStreamDB's windowed GROUP BY operators.
 *
 * What it replaces (reference = Yu-zh/hstream @ 2025-01-17, paths relative to
 * its root):
 *
 *   hsg_op_create (HSG_TUMBLING / HSG_HOPPING)
 *       TimeWindowedStream.aggregate / count
 *         hstream-processing/src/HStream/Processing/Stream/TimeWindowedStream.hs:32-70
 *       with the window spec of mkTumblingWindow / mkHoppingWindow
 *         .../Stream/TimeWindows.hs:23-43
 *   hsg_op_create (HSG_SESSION)
 *       SessionWindowedStream.aggregate / count
 *         .../Stream/SessionWindowedStream.hs:33-72, mkSessionWindows SessionWindows.hs:25-30
 *   hsg_op_create (HSG_UNWINDOWED)
 *       GroupedStream.aggregate / count  .../Stream/GroupedStream.hs:35-87
 *   hsg_push_batch
 *       the per-record processors TimeWindowedStream.aggregateProcessor (:72-117),
 *       SessionWindowedStream.aggregateProcessor (:74-118),
 *       GroupedStream.aggregateProcessor (:71-87), driven for a whole poll batch
 *       instead of record by record by runTask (Processor.hs:128-144), with the
 *       stream-time update of Processor.hs:139 / Processor/Internal.hs:160-166.
 *   hsg_drain
 *       the `forward` of every updated (key, window) row (TimeWindowedStream.hs:101,
 *       SessionWindowedStream.hs:97,118, GroupedStream.hs:87).
 *   hsg_dump_state
 *       ksDump / ssDump (Store.hs:59,81 and :143,238-241) used by views
 *       (hstream/src/HStream/Server/Handler.hs:274-321).
 *   hsg_view_get
 *       ksGet / findSessions / ssGet (Store.hs:59,243-272) and with them the one
 *       read of a view, SELECT ... FROM view WHERE key = x (SelectViewPlan,
 *       hstream/src/HStream/Server/Handler.hs:277-323), by key instead of from a dump.
 *   hsg_table_join
 *       Stream.joinTable / joinTableProcessor (.../Processing/Stream.hs:302-344): the
 *       ksGet per stream record, for a whole poll batch, against an unwindowed op.
 *   hsg_agg kinds
 *       the SQL aggregate components of hstream-sql/src/HStream/SQL/Codegen.hs:399-469
 *       (COUNT(*), COUNT(col), SUM, MIN, MAX, non-aggregate passthrough = HSG_LAST)
 *       plus AVG, which the reference rejects at codegen (Codegen.hs:462) and which
 *       this ABI defines as SUM(col) / COUNT(col).
 *
 * Conventions (mirroring the reference's own FFI, hstream-store cbits and
 * common/HStream/Stats.hs): opaque handles freed by *_destroy functions that
 * are usable as ForeignPtr finalizers, plain pointers + sizes, int status codes
 * (0 = OK, negative = error), no C++ exception crosses the ABI, a per-handle
 * last-error string. Calls on one op handle must be serialized by the caller;
 * distinct op handles may be used concurrently from different OS threads.
 * hsg_push_batch blocks until the GPU work is done: bind it as a *safe* ccall.
 */
#ifndef HSTREAM_GPU_H
#define HSTREAM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
#define HSG_OK           0
#define HSG_E_INVALID   (-1) /* bad argument / unsupported combination           */
#define HSG_E_OOM       (-2) /* HBM state table or session arena full            */
#define HSG_E_CAPACITY  (-3) /* batch larger than capacity / changelog not drained / out buffer too small */
#define HSG_E_DEVICE    (-4) /* HIP runtime error                                */
#define HSG_E_COMM      (-5) /* RCCL error                                       */
#define HSG_E_RANGE     (-6) /* window index outside the op's 2^32-window span   */

/* key id reserved for records that only advance stream time (filtered by WHERE,
 * failed decode, aggregate type error): Processor.hs:139 updates the task
 * timestamp before the topology runs, so such records still move the watermark. */
#define HSG_KEY_NONE 0xFFFFFFFFu

#define HSG_COMM_ID_BYTES 128

/* grace used by every reference window spec: 24 h (TimeWindows.hs:34,42; SessionWindows.hs:29) */
#define HSG_DEFAULT_GRACE_MS 86400000LL

enum hsg_window_kind {
  HSG_TUMBLING   = 0, /* mkTumblingWindow size            (advance = size)      */
  HSG_HOPPING    = 1, /* mkHoppingWindow size advance                           */
  HSG_SESSION    = 2, /* mkSessionWindows gap (grace unused, as in the reference) */
  HSG_UNWINDOWED = 3  /* GroupedStream.aggregate: one implicit window per key   */
};

enum hsg_emit_mode {
  HSG_EMIT_PER_RECORD = 0, /* exact reference changelog: one row per (record, accepted window),
                              arrival order, windows in ascending start              */
  HSG_EMIT_PER_BATCH  = 1, /* one row per group touched by the batch = the last per-record
                              row of that group; order unspecified                     */
  HSG_EMIT_NONE       = 2  /* state only (views)                                       */
};

enum hsg_col_type { HSG_I64 = 0, HSG_F64 = 1 };

enum hsg_agg_kind {
  HSG_COUNT_ALL = 0, /* COUNT(*)   Codegen.hs:404-411, DSL count TimeWindowedStream.hs:59-70 */
  HSG_COUNT     = 1, /* COUNT(col) Codegen.hs:412-422: +1 when the field is present          */
  HSG_SUM       = 2, /* SUM(col)   Codegen.hs:423-435                                        */
  HSG_MIN       = 3, /* MIN(col)   Codegen.hs:449-461, identity maxBound::Int                */
  HSG_MAX       = 4, /* MAX(col)   Codegen.hs:436-448, identity minBound::Int                */
  HSG_AVG       = 5, /* SUM(col)/COUNT(col) as f64 (NaN when COUNT(col) = 0; a HAVING program
                        reads that NaN as its error value, see "HAVING pushdown" below)      */
  HSG_LAST      = 6  /* non-aggregate SELECT column, Codegen.hs:463-469 (time windows and
                        unwindowed only)                                                     */
};

enum hsg_mem { HSG_MEM_HOST = 0, HSG_MEM_DEVICE = 1 };

/* Narrow transport encodings of a batch's columns (hsg_batch ts_enc / col_enc).
 * A poll batch crosses PCIe before any kernel sees it, so its bytes per record
 * bound a host-fed op's throughput; a producer that knows a column's range
 * (the decoder sees every value) may send it narrower. Lossless: the library
 * widens on the device before the batch runs. */
enum hsg_enc {
  HSG_ENC_FULL  = 0, /* the column's own type: int64 ts, int64 / double values          */
  HSG_ENC_TS32  = 1, /* ts only: int32 offsets from hsg_batch.ts_base                   */
  HSG_ENC_I32   = 2, /* an HSG_I64 column sent as int32 (every value fits)              */
  HSG_ENC_DEC32 = 3, /* an HSG_F64 column sent as int32 decimal mantissas m:
                        value = m / 10^col_scale, the double nearest that decimal,
                        i.e. the double the JSON text of the decimal parses to       */
  HSG_ENC_K16   = 4, /* key_id only: uint16 ids (a dictionary of <= 65536 keys, and
                        no HSG_KEY_NONE record in the batch)                        */
  HSG_ENC_TS16  = 5  /* ts only: uint16 offsets from per-frame bases (frame of
                        reference): record i's ts = ts_frames[i / HSG_TS16_FRAME] +
                        offset[i]; a poll batch's near-sorted timestamps fit when
                        every frame of HSG_TS16_FRAME records spans < 65536 ms     */
};
#define HSG_TS16_FRAME 4096

/* WHERE pushdown: the query's filter as a postfix program the op runs on the
 * GPU over each staged batch, ahead of the aggregate. The reference runs it as
 * a node of its own in front of the aggregate (genFilterNode whr s0,
 * hstream-sql/src/HStream/SQL/Codegen.hs:540) with the semantics of
 * genRExprValue / genFilterR (Codegen.hs:290-341); a record it drops -- or one
 * whose field lookup throws (getFieldByName, Internal/Codegen.hs:41-49) -- has
 * already moved stream time (Processor.hs:139-143), which here is: its key
 * becomes HSG_KEY_NONE. Nothing is compacted, so src_index keeps its meaning.
 *
 * A value is an i64 or an f64, typed statically by its column's type or its
 * constant's kind. ADD / SUB / MUL of two i64 is an i64 and wraps; with an f64
 * operand the result is an f64. An i64 is compared with an f64 exactly, as
 * Scientific values compare (2^53 + 1 > 9007199254740992.0): never through a
 * conversion of the integer to double. Evaluation is three-valued (true /
 * false / error), which is what Haskell's laziness makes of a missing field:
 *   COL        error when bit 0 of the record's valid byte is 0 (bit 1, the
 *              literal form, is not looked at)
 *   ADD..MUL   error if either operand is
 *   EQ..GE     error if either operand is
 *   BETWEEN    (lo x hi): error if lo or x is; else false if lo > x, whatever
 *              hi is; else error if hi is; else x <= hi
 *   OR         l true -> true; l error -> error; l false -> r
 *   AND        l false -> false; l error -> error; l true -> r
 *   NOT        NOT error = error
 * A record is kept only when the result is true. Both operands of AND / OR
 * are always computed (nothing has a side effect): the short circuit is a
 * rule on values. Not expressible, such a WHERE stays upstream of the op:
 * string / bool / null constants, predicates on the group key.
 *
 * FN (value -> value) applies the numeric function `arg` (hsg_fn), the
 * reference's unaryOpOnValue (Internal/Codegen.hs:139-179). Typing is static:
 *   ABS                  the operand's type; an i64 INT64_MIN wraps
 *   CEIL / FLOOR / ROUND the operand's type: the identity on an i64, on an f64
 *                        an f64 holding an integer; ROUND is half to even
 *   SIGN                 i64: -1, 0 or 1
 *   the other 17         f64; an i64 operand is converted with (double);
 *                        LOG2 / LOG10 are log(x) / log(2.0), log(x) / log(10.0)
 * The result is the error value (what an absent column is) when the operand
 * is, and where the reference throws "Mathematical error": ASIN / ACOS outside
 * [-1, 1], ACOSH below 1, ATANH outside (-1, 1), LOG / LOG2 / LOG10 at or
 * below 0 (an i64 operand is tested as an integer). It is also the error
 * value for SQRT of a negative number and for any function whose f64 operand
 * or f64 result is not finite (the reference makes a meaningless finite number
 * of those). */
enum hsg_fn {
  HSG_FN_SIN = 0, HSG_FN_SINH = 1, HSG_FN_ASIN = 2, HSG_FN_ASINH = 3,
  HSG_FN_COS = 4, HSG_FN_COSH = 5, HSG_FN_ACOS = 6, HSG_FN_ACOSH = 7,
  HSG_FN_TAN = 8, HSG_FN_TANH = 9, HSG_FN_ATAN = 10, HSG_FN_ATANH = 11,
  HSG_FN_ABS = 12, HSG_FN_CEIL = 13, HSG_FN_FLOOR = 14, HSG_FN_ROUND = 15, HSG_FN_SQRT = 16, HSG_FN_SIGN = 17,
  HSG_FN_LOG = 18, HSG_FN_LOG2 = 19, HSG_FN_LOG10 = 20, HSG_FN_EXP = 21
};
#define HSG_FN_COUNT 22
enum hsg_where_opcode {
  HSG_W_COL = 0,  /* push value column `arg`                                  */
  HSG_W_I64 = 1,  /* push imm.i                                               */
  HSG_W_F64 = 2,  /* push imm.f (finite)                                      */
  HSG_W_ADD = 3, HSG_W_SUB = 4, HSG_W_MUL = 5,        /* value value -> value */
  HSG_W_EQ = 6, HSG_W_NE = 7, HSG_W_LT = 8, HSG_W_GT = 9, HSG_W_LE = 10, HSG_W_GE = 11, /* value value -> bool */
  HSG_W_BETWEEN = 12,                                  /* lo x hi -> bool      */
  HSG_W_AND = 13, HSG_W_OR = 14, HSG_W_NOT = 15,       /* bool (bool) -> bool  */
  /* 16..31 are not opcodes */
  HSG_W_FN = 32                                        /* value -> value: hsg_fn `arg` */
};
typedef struct { int32_t op; int32_t arg; union { int64_t i; double f; } imm; } hsg_where_ins;
#define HSG_WHERE_MAX_INS   64
#define HSG_WHERE_MAX_DEPTH 8

/* HAVING pushdown: the same program over the rows an op emits. The reference
 * chains genFilteRNodeFromHaving behind an unwindowed GROUP BY (Codegen.hs:
 * 524-529, :561-566): genFilterR over each emitted record's aggregate object
 * {alias: Number}. Here the op filters, at the end of every push, the changelog
 * rows the batch appended, and compacts the rows it keeps in their order; only
 * those become pending (hsg_stats.pending_rows, hsg_pending_rows, hsg_drain),
 * with src_index unchanged -- a dropped record's row is simply absent.
 *
 * HSG_W_COL arg names aggregate `arg` of the op (cfg->aggs[arg]); its type is
 * static: HSG_COUNT_ALL and HSG_COUNT are i64, HSG_SUM / HSG_MIN / HSG_MAX /
 * HSG_LAST have their column's type, HSG_AVG is f64. The program reads the
 * 8-byte word the row carries, the reference's initial values included
 * (maxBound / minBound of a MIN / MAX nothing reached, 0 of a LAST): they are
 * Numbers and compare as such; literal forms are not looked at. Every alias
 * is in the object, so COL is never the error value -- with one exception the
 * engine defines, HSG_AVG not being in the reference: an f64 output that is
 * NaN (HSG_AVG with COUNT(col) = 0, see hsg_agg_kind) is the error value, and
 * the row is dropped unless an OR / AND / BETWEEN rule decides before it.
 * Everything else is the WHERE semantics above, unchanged. A row is kept only
 * when the result is true.
 *
 * HAVING filters the emitted rows only: the state, hsg_dump_state,
 * hsg_view_get, watermarks and the pairs / touched / late_dropped statistics
 * are those of the op without it (the reference's materialized store sits
 * before the filter). The reference ignores HAVING on a windowed GROUP BY
 * (Codegen.hs:554-559); this ABI is wider: any window kind with
 * HSG_EMIT_PER_RECORD or HSG_EMIT_PER_BATCH. The rows are written, then
 * compacted: the changelog room check ahead of a push (HSG_E_CAPACITY) stays
 * the batch's worst case before the filter. */

/* Computed columns: the SELECT list's value expressions, evaluated per record
 * ahead of the aggregate. The reference keeps, per group, genRExprValue of
 * the last record for any value expression of the SELECT list
 * (genAggregateComponentsFromDerivedCol, Codegen.hs:463-469); aggregates over
 * arithmetic, SUM(price * qty), are this engine's, as HSG_AVG is.
 *
 * A map is a list of value programs: hsg_where_ins sequences of HSG_W_COL,
 * HSG_W_I64, HSG_W_F64, HSG_W_ADD, HSG_W_SUB, HSG_W_MUL and HSG_W_FN only, each
 * leaving exactly one value. COL arg names a column of the batch (cfg->n_cols,
 * cfg->col_types), as in the WHERE program. Expression j defines the
 * aggregates' column j: with a map, cfg->aggs[].column indexes the
 * expressions, not the batch. An expression's type is static, i64 unless an
 * f64 column or constant takes part, and the arithmetic is the WHERE
 * program's (i64 wraps; with an f64 operand IEEE f64, one rounding per
 * instruction).
 *
 * An expression that reads a column whose valid bit 0 is clear is the error
 * value for that record. By default the derived column is then absent for
 * the record (bit 0 of its valid byte is 0) and every aggregate over it
 * leaves its accumulator alone, as for an absent bare column. With
 * HSG_MAP_STRICT on the expression the record is dropped instead: its key
 * becomes HSG_KEY_NONE after it has moved stream time, exactly as a WHERE
 * drop (the reference's strict HashMap forces genRExprValue, getFieldByName
 * throws inside aggregateF, and runTask goes on after
 * updateTimestampInTaskContext, Processor.hs:139-143).
 *
 * Ops with HSG_OPF_LITERAL_FORMS take bit 1 of the derived valid byte from
 * the operands: COL gives the input's bit 1, an I64 constant 0, an F64
 * constant 1 iff it is not integral (2.0 is 2e0 to Scientific), ADD / SUB /
 * MUL the OR of their operands (DESIGN.md 9 for the one case this misses).
 * FN: ABS keeps its operand's bit, CEIL / FLOOR / ROUND / SIGN clear it, every
 * other function sets it iff its result is not integral. Without the flag bit
 * 1 is 0.
 *
 * WHERE comes first, over the raw columns, then the map: a record WHERE
 * dropped is not counted by the map. An expression that is a single COL is
 * an alias: nothing is computed, the aggregates read the caller's column. */
#define HSG_MAP_STRICT 1u
#define HSG_MAP_MAX_EXPRS 8
#define HSG_MAP_MAX_INS   64   /* all expressions together */
typedef struct { const hsg_where_ins *prog; int32_t n; uint32_t flags; } hsg_map_expr;
typedef struct {
  uint64_t map_dropped;        /* keyed records of the last batch (this rank's ingest) that WHERE
                                  kept and a strict expression dropped                          */
  uint64_t map_dropped_total;
  uint32_t computed_cols;      /* expressions the map pass computes and stores                  */
  uint32_t aliased_cols;       /* expressions that are a caller's column (a single COL)         */
} hsg_map_stats;

/* Scalar SELECT: WHERE, the SELECT list and HAVING of a query without GROUP
 * BY. The reference compiles SELECT a + b AS s, SQRT(c) AS r FROM src WHERE
 * x > 3 EMIT CHANGES to a chain of stateless nodes (the RGroupByEmpty branch of
 * genStreamBuilderWithStream, hstream-sql/src/HStream/SQL/Codegen.hs:542-550):
 * genFilterNode whr, genMapNode sel, genFilteRNodeFromHaving hav, then the
 * sink. A select op (hsg_op_create_select) is that chain for a whole poll
 * batch: it keeps no state and has no group key. Per record, in arrival order:
 *
 *   1. A record whose key_id is HSG_KEY_NONE is skipped (it still moves stream
 *      time). hsg_batch.key_id may be NULL for a select op: then every record
 *      is live and its row carries HSG_KEY_NONE.
 *   2. WHERE, the program above unchanged, over the raw columns; the record is
 *      kept only on true. n_where == 0: every record is kept.
 *   3. Expression j (a value program as in a map, 0 <= n_exprs <=
 *      HSG_MAP_MAX_EXPRS, HSG_MAP_MAX_INS for all together) gives column j of
 *      the row. Every expression is strict, whatever its flags say: the
 *      reference builds the mapped object with Data.HashMap.Strict.fromList
 *      (Codegen.hs:13, :349-353), so a missing field throws and runTask drops
 *      the record. A record with any error expression emits no row.
 *   4. HAVING, the same condition program with HSG_W_COL arg = expression arg,
 *      typed by the expression's static type; an f64 value that is NaN is the
 *      error value (the HAVING rule above). The row is kept only on true.
 *      n_having == 0: every row is kept.
 *   5. Kept rows are appended to the changelog, compacted, in arrival order:
 *      key_id the record's, win_start = win_end = its ts (genMapR keeps the
 *      record's timestamp), src_index the global index of the record (records
 *      pushed since create / reset, as in every per-record changelog),
 *      aggs[j] = expression j and hsg_rows.n_aggs = n_exprs. With
 *      HSG_OPF_LITERAL_FORMS bit 2j of `form` is set iff expression j prints
 *      as an integer: iff the derived bit 1 of "Computed columns" above is
 *      clear (no operand had a literal with a negative exponent, or the rules
 *      for constants and functions there); bit 2j + 1 is always 0. Without
 *      the flag rows carry no form.
 *
 * n_exprs == 0 is SELECT * ... WHERE: the rows carry src_index only and the
 * host forwards the original records by index.
 *
 * Stream time moves as for every op (inout_watermark, hsg_stats.records /
 * batches). The room check comes ahead of the push and is the batch's worst
 * case: pending + n > out_capacity gives HSG_E_CAPACITY and nothing is
 * applied. The op has no state: hsg_state_rows gives 0, hsg_dump_state,
 * hsg_view_get and hsg_table_join HSG_E_INVALID; every other call on an op
 * works as on any op. On a sharded engine the op is local: no exchange, no
 * collective, each rank filters its own slice. */
typedef struct {
  int32_t n_cols;           /* value columns carried by every batch (<= 8)                */
  uint32_t flags;           /* HSG_OPF_LITERAL_FORMS or 0                                  */
  const int32_t *col_types; /* n_cols hsg_col_type                                         */
  uint64_t out_capacity;    /* changelog rows buffered between drains; 0 = the engine's
                               batch_capacity                                             */
} hsg_select_config;
typedef struct {
  uint64_t where_dropped;   /* live records of the last batch WHERE dropped                */
  uint64_t where_dropped_total;
  uint64_t expr_dropped;    /* ... WHERE kept and an expression's error value dropped      */
  uint64_t expr_dropped_total;
  uint64_t having_dropped;  /* ... both kept and HAVING dropped                            */
  uint64_t having_dropped_total;
  uint64_t emitted;         /* rows the last batch appended                                */
  uint64_t emitted_total;
} hsg_select_stats;

typedef struct hsg_engine hsg_engine;
typedef struct hsg_op hsg_op;

/* transports of the key exchange */
#define HSG_TRANSPORT_RCCL 0  /* one process per GPU over RCCL (xGMI)                       */
#define HSG_TRANSPORT_HOST 1  /* ranks of one host through shared memory (several ranks may
                                 share one GPU): for testing the multi-rank sequencing    */

typedef struct {
  int32_t device;          /* HIP device ordinal; -1 = the calling thread's current device */
  int32_t rank;            /* this process's rank in the key-sharded group                */
  int32_t nranks;          /* 1 = single GPU, no communicator                              */
  int32_t transport;       /* HSG_TRANSPORT_RCCL (0) or HSG_TRANSPORT_HOST                  */
  const uint8_t *comm_id;  /* RCCL: HSG_COMM_ID_BYTES from hsg_comm_unique_id() on rank 0,
                              shared out of band; HOST: a NUL-terminated segment name (the
                              same on every rank, no '/'); NULL when nranks == 1           */
  uint64_t batch_capacity; /* max records per hsg_push_batch on this rank                   */
} hsg_engine_config;

typedef struct {
  int32_t kind;   /* hsg_agg_kind                                  */
  int32_t column; /* value column index; ignored for HSG_COUNT_ALL */
} hsg_agg;

typedef struct {
  int32_t window_kind;     /* hsg_window_kind                                            */
  int32_t emit_mode;       /* hsg_emit_mode                                              */
  int64_t size_ms;         /* TUMBLING / HOPPING window size  (twSizeMs)                 */
  int64_t advance_ms;      /* HOPPING advance (twAdvanceMs); TUMBLING: = size_ms         */
  int64_t gap_ms;          /* SESSION inactivity gap (swInactivityGap)                   */
  int64_t grace_ms;        /* twGraceMs; use HSG_DEFAULT_GRACE_MS for reference parity  */
  int32_t n_cols;          /* value columns carried by every batch                       */
  int32_t n_aggs;
  const int32_t *col_types;/* n_cols hsg_col_type                                        */
  const hsg_agg *aggs;     /* n_aggs output aggregates, in output order                  */
  uint64_t state_capacity; /* HBM state rows (groups or sessions) to start with; 0 = engine
                            * default (2^21). Time-window tables then grow before a batch
                            * that could pass 3/4 load: by the groups the batch makes on
                            * the lean one-window path (which checks and, if short of
                            * room, grows and runs the batch again), else by one group
                            * per (record, window)                                      */
  uint64_t out_capacity;   /* changelog rows buffered in HBM between drains; 0 = default */
  uint32_t flags;          /* HSG_OPF_* (0 = none)                                        */
  uint32_t reserved;       /* 0                                                           */
} hsg_op_config;

/* hsg_op_config.flags */
#define HSG_OPF_LITERAL_FORMS 1u /* Track how aeson prints each SUM / MIN / MAX / LAST output:
   the reference aggregates Data.Scientific values, and aeson prints a Scientific
   whose exponent is >= 0 as an integer, else in Generic form ("6" vs "6.0",
   hstream-sql/src/HStream/SQL/Codegen/Boilerplate.hs:32-37 objectSerde over
   Codegen.hs:423-469). Batches then mark, in bit 1 of each valid byte, the values
   whose JSON literal had a negative exponent (hstream_ingest.h literal_forms); a
   SUM prints as an integer iff none of its values did (a Scientific sum takes the
   smaller exponent), a MIN / MAX / LAST as its winning literal was spelled, an
   aggregate nothing reached as the reference's initial value. Ties between equal
   values spelled differently (7 and 7.0) resolve as the reference's folds do:
   a time window's or a session's record fold keeps the earlier literal for MIN
   and takes the later for MAX (min n x = n, max n x = x, Codegen.hs:442,455); a
   session merge keeps the merged side's for MIN and takes the existing
   session's for MAX (min n1 n2 / max n1 n2, Codegen.hs:447,460). Changelog and
   dump rows then carry hsg_rows.form. Any number of value columns; such ops run
   on the generic record kernels (the fast partition layouts carry no literal
   bits). */

/* One micro-batch in columnar form, records in arrival order.
 *
 * Device-resident batches (mem = HSG_MEM_DEVICE) are read on the op's own HIP
 * stream, which is not ordered after the stream that produced them: either
 * the producer's writes are complete when hsg_push_batch is called (e.g. the
 * producer synchronised its stream), or ready_event names a hipEvent_t
 * recorded on the producing stream after its last write, and the op's stream
 * waits on it before reading. Host batches are copied to the device inside
 * the call (sync) or before completion is signalled (async). */
typedef struct {
  uint64_t n;
  int32_t mem;                  /* hsg_mem of every pointer below                        */
  int32_t n_cols;               /* must equal the op's n_cols                            */
  const uint32_t *key_id;       /* dictionary-encoded group-by key, HSG_KEY_NONE = skip
                                   (a select op's batch: may be NULL, every record live)  */
  const int64_t *ts;            /* event timestamp, ms (record header publish time)      */
  const void *const *cols;      /* n_cols arrays of int64_t or double                    */
  const uint8_t *const *valid;  /* n_cols presence arrays (1 byte/record, 0 = field absent);
                                   NULL or a NULL entry = all present                    */
  void *ready_event;            /* optional hipEvent_t the op's stream waits on (device
                                   batches); NULL = inputs already complete              */
  /* narrow transport (all zero = the full-width arrays above) */
  int32_t ts_enc;               /* HSG_ENC_FULL, HSG_ENC_TS32 (`ts` points at int32_t[n]) or
                                   HSG_ENC_TS16 (`ts` points at uint16_t[n], + ts_frames) */
  int32_t key_enc;              /* HSG_ENC_FULL, or HSG_ENC_K16: `key_id` points at uint16_t[n] */
  int64_t ts_base;              /* HSG_ENC_TS32: ts of a record = ts_base + its offset     */
  uint8_t col_enc[8];           /* per value column: HSG_ENC_FULL, HSG_ENC_I32 (HSG_I64
                                   columns) or HSG_ENC_DEC32 (HSG_F64 columns)            */
  uint8_t col_scale[8];         /* HSG_ENC_DEC32: decimal digits after the point, <= 18   */
  const int64_t *ts_frames;     /* HSG_ENC_TS16: ceil(n / HSG_TS16_FRAME) frame bases (the
                                   batch's hsg_mem); NULL otherwise                       */
} hsg_batch;

/* Columnar changelog / state rows. */
typedef struct {
  uint64_t capacity;   /* rows every array can hold                                    */
  int32_t mem;         /* hsg_mem of every pointer below                               */
  int32_t n_aggs;      /* must equal the op's n_aggs                                   */
  uint32_t *key_id;
  int64_t *win_start;  /* time windows: window start; sessions: session start          */
  int64_t *win_end;    /* time windows: start + size; sessions: session end (inclusive) */
  int64_t *src_index;  /* per-record mode: global index of the producing record; else -1 */
  void *const *aggs;   /* n_aggs arrays: int64_t (COUNT*, SUM/MIN/MAX/LAST of i64) or double */
  uint32_t *form;      /* optional (NULL = not wanted), ops with HSG_OPF_LITERAL_FORMS:
                          per row, bits 2j / 2j+1 of aggregate j: aeson prints it as an
                          integer / it is the aggregate's initial value (nothing reached it) */
} hsg_rows;

typedef struct {
  uint64_t batches;           /* batches pushed since create/reset                     */
  uint64_t records;           /* records pushed (this rank's ingest)                    */
  uint64_t records_owned;     /* records aggregated on this rank after the key exchange */
  uint64_t pairs;             /* accepted (record, window) updates, last batch          */
  uint64_t late_dropped;      /* (record, window) pairs rejected by grace, last batch   */
  uint64_t touched;           /* groups / sessions touched, last batch                  */
  uint64_t state_rows;        /* live groups / sessions                                 */
  uint64_t pending_rows;      /* changelog rows waiting for hsg_drain                   */
  double   last_batch_ms;     /* wall time of the last hsg_push_batch                   */
  double   agg_kernel_ms;     /* cumulative device time of the dominant kernel          */
  uint64_t agg_kernel_launches;
  double   exchange_ms;       /* cumulative device time of the key exchange             */
  uint64_t exchange_bytes;    /* cumulative bytes this rank sent to peers               */
  uint64_t pairs_total;       /* cumulative accepted (record, window) updates           */
  uint64_t touched_total;     /* cumulative groups / sessions touched (summed per batch) */
  uint64_t state_slots;       /* 8-byte aggregate words per state row (the op's program) */
  uint64_t state_row_bytes;   /* algorithmic state row: group key 8 B + 8 B per slot
                                 (sessions: start + end + slots)                        */
  uint64_t spilled_rows;      /* closed windows kept in host memory (counted in state_rows;
                                 hsg_dump_state returns them after the HBM rows)        */
  uint64_t spill_events;      /* retention passes that moved closed windows to the host */
  uint64_t table_slots;       /* HBM hash-table slots (time windows) / key-table slots
                                 (sessions) now                                          */
  uint64_t grow_events;       /* times the HBM table was rebuilt larger                   */
  uint64_t lean_batches;      /* batches aggregated by the lean one-window path            */
  uint64_t direct_batches;    /* ... whose changelog rows the lean apply wrote itself      */
  uint64_t replays;           /* batches completed after the fetch because the predicted
                                 kernel variants did not match the batch (speed only)     */
  uint64_t overflow_rows;     /* groups in the table's overflow rows now: a key-hash region
                                 was full when they were claimed (skewed keys, or keys with
                                 many open windows); the next batch rebuilds the table    */
  uint64_t overflow_rebuilds; /* table rebuilds (twice the slots, twice the region size)
                                 that overflow rows caused                               */
  uint64_t where_dropped;     /* records of the last batch (this rank's ingest) that arrived
                                 keyed and were masked by the op's WHERE program          */
  uint64_t where_dropped_total;
  uint64_t having_dropped;    /* changelog rows of the last batch (this rank's) that the op's
                                 HAVING program removed before they became pending        */
  uint64_t having_dropped_total;
} hsg_stats;

/* Completion callback of hsg_push_batch_async: rc is what hsg_push_batch
 * would have returned. Runs on the op's completion thread; it must not call
 * back into the same op. The Haskell binding passes a C shim that stores rc
 * and calls hs_try_putmvar(cap, mvar), the pattern of
 * hstream-store/cbits/logdevice/hs_writer.cpp:29-44. */
typedef void (*hsg_done_fn)(void *ctx, int rc);

/* ---- engine: one per process and GPU ---------------------------------------- */
int  hsg_comm_unique_id(uint8_t *out, size_t len);
int  hsg_engine_create(const hsg_engine_config *cfg, hsg_engine **out);
void hsg_engine_destroy(hsg_engine *eng);
const char *hsg_engine_last_error(const hsg_engine *eng);

/* ---- operator: one per windowed GROUP BY -------------------------------------- */
int  hsg_op_create(hsg_engine *eng, const hsg_op_config *cfg, hsg_op **out);
/* Type-check a WHERE program against an op's value columns; pure host code
 * (no GPU). HSG_OK only when every operand has the kind its instruction takes
 * (value or bool), the stack never holds more than HSG_WHERE_MAX_DEPTH
 * entries, exactly one bool is left at the end, every column is in range,
 * 1 <= n <= HSG_WHERE_MAX_INS and every f64 constant is finite; else
 * HSG_E_INVALID with a message in err (NUL-terminated, cut to err_len). */
int  hsg_where_check(const hsg_where_ins *prog, int32_t n, const int32_t *col_types, int32_t n_cols, char *err,
                     size_t err_len);
/* hsg_op_create with a WHERE program of n instructions (n == 0: none; that is
 * hsg_op_create). Every batch then carries cfg->n_cols columns as before: the
 * ones the aggregates read and the ones only the program reads, which leave
 * the batch once the filter ran (the op aggregates as the op without them
 * would). The program is copied and fixed for the op's life; hsg_op_reset
 * keeps it. A program hsg_where_check refuses fails the creation with
 * HSG_E_INVALID and that message in hsg_engine_last_error. Collective on a
 * sharded engine, like hsg_op_create. */
int  hsg_op_create_where(hsg_engine *eng, const hsg_op_config *cfg, const hsg_where_ins *prog, int32_t n,
                         hsg_op **out);
/* Type-check a HAVING program against the op's aggregate outputs; pure host
 * code (no GPU). As hsg_where_check, with every column in [0, cfg->n_aggs)
 * and typed as above; the messages begin "having: ". */
int  hsg_having_check(const hsg_where_ins *prog, int32_t n, const hsg_op_config *cfg, char *err, size_t err_len);
/* hsg_op_create with a WHERE program (n_where == 0: none) and a HAVING program
 * (n_having == 0: none); with both 0 it is hsg_op_create, with n_having == 0
 * hsg_op_create_where. The programs are copied and fixed for the op's life;
 * hsg_op_reset keeps them. HSG_E_INVALID (message in hsg_engine_last_error)
 * for a program its check refuses, and for a HAVING program on an
 * HSG_EMIT_NONE op, which has nothing to filter. Collective on a sharded
 * engine, like hsg_op_create; the filter itself is local to each rank's rows. */
int  hsg_op_create_filtered(hsg_engine *eng, const hsg_op_config *cfg, const hsg_where_ins *where, int32_t n_where,
                            const hsg_where_ins *having, int32_t n_having, hsg_op **out);
/* Rows of one compaction tile of the HAVING pass (tests size their segments by it). */
int  hsg_having_tile_rows(void);
/* Type-check a map (hsg_map_expr, above) against an op's value columns; pure
 * host code (no GPU). HSG_OK, with out_types[j] (may be null) the static type
 * of expression j, only when 1 <= n_exprs <= HSG_MAP_MAX_EXPRS, the programs
 * hold at most HSG_MAP_MAX_INS instructions together, every opcode is one of
 * COL / I64 / F64 / ADD / SUB / MUL / FN, every program leaves exactly one value
 * and never holds more than HSG_WHERE_MAX_DEPTH, every column is in range and
 * every f64 constant is finite; else HSG_E_INVALID with a message in err that
 * begins "map: " ("map: expr <j>: " for a fault of expression j). */
int  hsg_map_check(const hsg_map_expr *exprs, int32_t n_exprs, const int32_t *col_types, int32_t n_cols,
                   int32_t *out_types, char *err, size_t err_len);
/* hsg_op_create_filtered with a map of n_exprs expressions (n_exprs == 0:
 * none; that is hsg_op_create_filtered). cfg->n_cols / col_types describe the
 * batch, the WHERE program and the expressions number its columns alike, and
 * cfg->aggs[].column indexes the expressions, typed as hsg_map_check types
 * them; the HAVING program is checked against those types ("having: ..." in
 * hsg_engine_last_error). The programs are copied and fixed for the op's
 * life; hsg_op_reset keeps them. A map hsg_map_check refuses fails the
 * creation with HSG_E_INVALID and that message in hsg_engine_last_error.
 * Collective on a sharded engine, like hsg_op_create: each rank maps its own
 * slice before the exchange, which then carries the derived columns only. */
int  hsg_op_create_mapped(hsg_engine *eng, const hsg_op_config *cfg, const hsg_map_expr *exprs, int32_t n_exprs,
                          const hsg_where_ins *where, int32_t n_where,
                          const hsg_where_ins *having, int32_t n_having, hsg_op **out);
/* The map's counters (hsg_stats keeps its size); zeros for an op without one. */
int  hsg_op_map_stats(const hsg_op *op, hsg_map_stats *out);
/* Threads of one resident round of the map pass's grid: a batch of more records
 * strides (tests size a batch past it). */
int  hsg_map_grid_threads(void);
/* The function class of a program; pure host code (no GPU): 0 = no HSG_W_FN,
 * 1 = only ABS / CEIL / FLOOR / ROUND / SIGN / SQRT (the exact family), 2 =
 * any other function. Each pass has one kernel per class, and an op runs the
 * class of its programs: today's programs run today's kernels. */
int  hsg_prog_fn_class(const hsg_where_ins *prog, int32_t n);
/* hsg_map_grid_threads of the map pass's kernel of function class fn_class
 * (0: hsg_map_grid_threads itself); 0 for a class that does not exist. */
int  hsg_map_grid_threads_fn(int fn_class);
/* Type-check the programs of a select op ("Scalar SELECT" above) against its
 * value columns; pure host code (no GPU). where / having: hsg_where_check's
 * rules (n == 0: none), the HAVING program's columns being the expressions,
 * typed as hsg_map_check types them; exprs: hsg_map_check's rules, with
 * n_exprs == 0 allowed. The messages begin "where: ", "map: " and "having: ";
 * bad columns give "select: ...". */
int  hsg_select_check(const hsg_where_ins *where, int32_t n_where, const hsg_map_expr *exprs, int32_t n_exprs,
                      const hsg_where_ins *having, int32_t n_having, const int32_t *col_types, int32_t n_cols,
                      char *err, size_t err_len);
/* Create a select op. The programs are copied and fixed for the op's life;
 * hsg_op_reset keeps them (and the cumulative counters) and drops the pending
 * rows. HSG_E_INVALID with hsg_select_check's message in
 * hsg_engine_last_error for programs it refuses, for a NULL cfg and for flags
 * other than HSG_OPF_LITERAL_FORMS. Not collective. */
int  hsg_op_create_select(hsg_engine *eng, const hsg_select_config *cfg, const hsg_where_ins *where, int32_t n_where,
                          const hsg_map_expr *exprs, int32_t n_exprs, const hsg_where_ins *having, int32_t n_having,
                          hsg_op **out);
/* The select op's counters (hsg_stats keeps its size); HSG_E_INVALID for any other op. */
int  hsg_op_select_stats(const hsg_op *op, hsg_select_stats *out);
int  hsg_select_tile_rows(void);    /* records per tile of the kernel                        */
int  hsg_select_grid_groups(void);  /* most workgroups one launch starts (function class 0):
                                       a batch of more tiles has workgroups take a second   */
void hsg_op_destroy(hsg_op *op);
int  hsg_op_reset(hsg_op *op);            /* drop all state and pending rows          */
const char *hsg_last_error(const hsg_op *op);

/* Process one batch. *inout_watermark is the task's stream time (initially -1,
 * Processor/Internal.hs:151); it is read as the value before the batch and
 * overwritten with the value after it (max over all ranks' records). */
int  hsg_push_batch(hsg_op *op, const hsg_batch *batch, int64_t *inout_watermark);

/* Asynchronous hsg_push_batch: validates and queues the batch, returns at
 * once (HSG_OK = queued, or an argument error). Queued batches of one op run
 * in call order on the op's completion thread; *inout_watermark is read when
 * the batch starts (so consecutive pushes may share one watermark variable)
 * and written before done(ctx, rc) is called. The batch's arrays (not the
 * hsg_batch struct itself, which is copied) must stay valid until done runs.
 * Any other call on the op first waits for the queue to drain. Bind as an
 * unsafe ccall: it never blocks on the GPU. */
int  hsg_push_batch_async(hsg_op *op, const hsg_batch *batch, int64_t *inout_watermark, hsg_done_fn done,
                          void *ctx);
/* Block until every queued asynchronous push of the op has completed; returns
 * the first non-OK status among them (HSG_OK if none), and clears it. */
int  hsg_op_wait(hsg_op *op);

int  hsg_pending_rows(const hsg_op *op, uint64_t *n);
/* Move up to out->capacity pending changelog rows into out (oldest first). If
 * the pending rows do not fit, copies nothing, sets *n_out to the number
 * pending and returns HSG_E_CAPACITY. */
int  hsg_drain(hsg_op *op, hsg_rows *out, uint64_t *n_out);

/* Zero-copy changelog: register caller-owned DEVICE columns (every column,
 * capacity rows) that pushes then write their changelog rows into directly, at
 * the pending offset; hsg_drain only reports and resets the pending count
 * (rows are at [0, n) of the registered columns; `out` may be NULL). NULL
 * restores the op's own buffer. Pending rows must be drained first. No
 * counterpart in the reference, whose forward hands rows to the sink one by
 * one (Processor.hs:221-266); here it saves a device copy per drain. */
int  hsg_op_set_changelog(hsg_op *op, const hsg_rows *dst);

int  hsg_state_rows(hsg_op *op, uint64_t *n);
/* Copy every live state row (views). Same capacity rule as hsg_drain. */
int  hsg_dump_state(hsg_op *op, hsg_rows *out, uint64_t *n_out);

/* Keyed view read: every live state row whose key_id is among key_ids[0,
 * n_keys) (host memory), the rows hsg_dump_state returns for those keys and
 * in its order (key_id, win_start, win_end), src_index -1, form filled for
 * ops with HSG_OPF_LITERAL_FORMS; out may be host or device memory. This is
 * the reference's one read of a view, SELECT ... FROM view WHERE key = x
 * (SelectViewPlan, hstream/src/HStream/Server/Handler.hs:277-323): ksGet for
 * an unwindowed key (at most one row, win_start = win_end = 0), the key's
 * windows (resident rows, overflow rows and the closed windows kept on the
 * host, merged), or its sessions in start order. The GPU reads the keys'
 * key-hash regions of the table (or their entries of the session key table),
 * not the table: cost follows the keys asked for, not the state's size.
 *
 * Duplicates count once; HSG_KEY_NONE, ids never pushed and keys another rank
 * owns match nothing. n_keys == 0 gives 0 rows; n_keys > HSG_VIEW_MAX_KEYS or
 * a NULL key_ids with n_keys > 0 gives HSG_E_INVALID. Same capacity rule as
 * hsg_drain: if the rows do not fit, nothing is written, *n_out is the number
 * needed (counted before any row is written, so a retry with that capacity
 * succeeds) and the call returns HSG_E_CAPACITY.
 *
 * The call changes nothing: not state, pending changelog rows, registered
 * changelog columns or hsg_stats. Like every call on an op it first waits for
 * the op's queued asynchronous pushes, and it is serialised with the op's
 * other calls by the caller. On a sharded engine it is NOT collective (no
 * RCCL call, no host-transport step): a rank answers for the keys it owns and
 * the caller unites the ranks' answers. */
#define HSG_VIEW_MAX_KEYS 1024
int  hsg_view_get(hsg_op *op, const uint32_t *key_ids, uint32_t n_keys, hsg_rows *out, uint64_t *n_out);

/* Stream-table join: the keys of one poll batch of the stream side, probed
 * against the state of an HSG_UNWINDOWED op, the Table that
 * GroupedStream.aggregate returns (GroupedStream.hs:53-56). This is the
 * reference's Stream.joinTable (hstream-processing/src/HStream/Processing/
 * Stream.hs:302-344): joinTableProcessor does ksGet key tableStore per stream
 * record, forwards joiner recordValue v2 on a hit and nothing on a miss. */
typedef struct {
  uint64_t n;              /* stream records of this poll batch, arrival order        */
  int32_t  mem;            /* hsg_mem of key_id                                       */
  int32_t  reserved;       /* 0                                                       */
  const uint32_t *key_id;  /* the stream's key in the TABLE op's dictionary;
                              HSG_KEY_NONE = no key, matches nothing                  */
  void *ready_event;       /* as hsg_batch.ready_event (device keys)                  */
} hsg_probe;

/* One output row per probe record whose key has a live row in `table`, in
 * arrival order: key_id is the record's key, win_start = win_end = 0,
 * src_index the record's index in the probe batch (0 .. n-1; the caller's
 * joiner pairs the stream record with the row through it), aggs[j] and form
 * what hsg_view_get returns for that key. out may be host or device memory;
 * device columns are written in place. Duplicate keys each get their own row;
 * HSG_KEY_NONE, ids never pushed and keys another rank owns match nothing.
 * Cost follows the probe batch (one table row read per record), not the
 * state's size.
 *
 * Only HSG_UNWINDOWED ops are tables (joinTableProcessor calls
 * getKVStateStore; window and session stores are not KV stores): any other
 * window kind gives HSG_E_INVALID. So do a NULL table, probe or n_out, a NULL
 * key_id with n > 0, n above the engine's batch_capacity, and reserved != 0.
 * n == 0 gives HSG_OK with 0 rows. Same capacity rule as hsg_drain: if the
 * matches do not fit out->capacity, nothing is written, *n_out is the number
 * needed (counted before any row is written, so a retry with that capacity
 * succeeds) and the call returns HSG_E_CAPACITY.
 *
 * The call reads only: state, pending changelog rows, registered changelog
 * columns, hsg_stats and the watermark are untouched (the reference's join
 * processor has no stream-time effect). Like every call on an op it first
 * waits for the op's queued asynchronous pushes, and it is serialised with
 * the op's other calls by the caller. On a sharded engine it is NOT
 * collective: a rank answers for the keys it owns. */
int  hsg_table_join(hsg_op *table, const hsg_probe *probe, hsg_rows *out, uint64_t *n_out);
/* Records per compaction tile of the join's kernels (tests size their shapes by it). */
int  hsg_table_join_tile(void);

/* Counters are cumulative since hsg_op_create (hsg_op_reset keeps them);
 * "last batch" fields describe the most recent hsg_push_batch. */
int  hsg_op_stats(const hsg_op *op, hsg_stats *out);

/* ---- testing hooks (not used by the drop-in) ----------------------------------
 * Process-wide knobs that let tests reach rare paths at small sizes; they apply
 * to ops created afterwards. Production code never sets them (defaults). */
#define HSG_KNOB_XPART_LOG2     1 /* a 1-rank exchange partitions its records into 2^v owner
                                     regions, all its own (0..6); -1 = log2(ranks)          */
#define HSG_KNOB_SESS_ARENA_MIN 2 /* floor of the session arena in rows (> 0); 0 = 2^20      */
#define HSG_KNOB_X_CLASSIC      3 /* 1: sequenced batches of a sharded op take the packed
                                     classic exchange instead of the columnar one            */
int  hsg_testing_set_knob(int32_t knob, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* HSTREAM_GPU_H */
