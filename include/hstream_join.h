/* libhstream_gpu — stream-stream join within a time window, on the GPU.
 *
 * Replaces joinStream / joinStreamProcessor
 * (hstream-processing/src/HStream/Processing/Stream.hs:222-300) over the two
 * InMemoryTimestampedKVStores (Store.hs:316-385) that the SQL
 * `s1 INNER JOIN s2 WITHIN (INTERVAL ...) ON s1.a = s2.b` plan builds
 * (hstream-sql/src/HStream/SQL/Codegen.hs:219-265). Per record, in arrival
 * order over both streams, the reference
 *   1. stores the record in its side's store under (record key, timestamp),
 *      replacing an entry with the same key and timestamp,
 *   2. range-scans the other side's store for the same record key over
 *      [ts - before, ts + after] (this side; the other side swaps before and
 *      after), in ascending timestamp,
 *   3. forwards, for every candidate whose join key equals the record's,
 *      (join key, joiner(this value, other value), max of the timestamps).
 * Two quirks of the reference are kept: the scan includes its end points
 * only when the other store holds some entry (any key) at both end
 * timestamps, else neither (tksRange's Maybe-chained splitLookup,
 * Store.hs:365-372); and a record or candidate without the join field
 * (HSG_KEY_NONE here) ends that record's scan at the first candidate, where
 * the reference's key selector throws (Codegen.hs:241-243; runTask's catch,
 * Processor.hs:140-143).
 *
 * Values stay with the caller: each record carries a 64-bit handle, and the
 * output rows name the two handles the joiner combines. The stores are never
 * pruned, as in the reference. A valued join (hsg_join_create_valued, below)
 * keeps the records' numeric value columns itself and drains joined rows.
 */
#ifndef HSTREAM_JOIN_H
#define HSTREAM_JOIN_H

#include "hstream_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int64_t before_ms;        /* JoinWindows jwBeforeMs (SQL: the WITHIN interval) */
  int64_t after_ms;         /* JoinWindows jwAfterMs                             */
  uint64_t batch_capacity;  /* records per push (both sides together)            */
} hsg_join_config;

/* one poll batch, both streams interleaved in arrival order */
typedef struct {
  uint64_t n;
  int32_t mem;                /* hsg_mem of every array                               */
  int32_t reserved0;
  const uint8_t *side;        /* 0 = this stream (left), 1 = the other stream         */
  const uint32_t *key_id;     /* record key (the stores' key), dictionary-encoded     */
  const uint32_t *join_key;   /* join key ({"SelectedKey": field}); HSG_KEY_NONE =
                                 the field is missing                                */
  const int64_t *ts;
  const uint64_t *handle;     /* the caller's reference to the record's value         */
} hsg_join_batch;

/* output rows: joiner(this value, other value) under join_key at ts */
typedef struct {
  uint64_t capacity;
  int32_t mem;
  int32_t reserved0;
  uint64_t *this_handle;
  uint64_t *other_handle;
  uint32_t *join_key;
  int64_t *ts;                /* max of the two records' timestamps */
} hsg_join_rows;

typedef struct hsg_join hsg_join;
int  hsg_join_create(hsg_engine *eng, const hsg_join_config *cfg, hsg_join **out);
void hsg_join_destroy(hsg_join *j);
const char *hsg_join_last_error(const hsg_join *j);
/* Records with key_id == HSG_KEY_NONE are dropped (the reference throws
 * before storing them). Output rows queue until hsg_join_drain. */
int  hsg_join_push(hsg_join *j, const hsg_join_batch *b);
int  hsg_join_pending(const hsg_join *j, uint64_t *n);
/* Same capacity rule as hsg_drain. */
int  hsg_join_drain(hsg_join *j, hsg_join_rows *out, uint64_t *n_out);
/* entries held by the two stores together */
int  hsg_join_state_rows(const hsg_join *j, uint64_t *n);

/* ---- valued join: the join keeps the records' value columns in HBM and
 * drains joined rows as the arrays of an hsg_batch -------------------------
 *
 * The reference's joiner for the SQL plan (genJoiner, hstream-sql/src/HStream/
 * SQL/Internal/Codegen.hs:62-67) is the union of both values under the field
 * names "s1.f" / "s2.g"; here a joined row is this side's columns followed by
 * the other side's, whichever side's record arrived last. A record's handle is
 * its value row: the number of records pushed to this join before it (every
 * record takes a row, also one without a record key), so hsg_join_drain still
 * works on a valued join and returns row numbers. The value rows are never
 * pruned, as the stores are not.
 *
 * Single rank only: on an engine with nranks > 1 hsg_join_create_valued
 * returns HSG_E_INVALID, before any collective and alike on every rank.
 * Numeric columns only (hsg_col_type). */
#define HSG_JOIN_MAX_COLS 8   /* both sides together: hsg_batch's limit */

typedef struct {
  int32_t n_cols[2];          /* [0] this side, [1] the other side; 0..8 each,
                                 at most HSG_JOIN_MAX_COLS together            */
  int32_t col_types[2][8];    /* hsg_col_type of each side's columns           */
} hsg_join_values;

/* the value columns of one hsg_join_batch, in the batch's mem */
typedef struct {
  const void *const *cols;      /* max(n_cols) arrays of batch->n int64_t or double:
                                   record i reads the first n_cols[side[i]] of them */
  const uint8_t *const *valid;  /* presence bytes (bit 0 present, bit 1 decimal
                                   literal); NULL or a NULL entry = all present  */
} hsg_join_cols;

/* joined rows: caller-owned arrays of `capacity` rows, host or device */
typedef struct {
  uint64_t capacity;
  int32_t mem;
  int32_t key_col;            /* key_id: -1 = the join key (the joined record's
                                 recordKey, Stream.hs:299); k >= 0 = joined column
                                 k (HSG_I64) as a dictionary id, HSG_KEY_NONE when
                                 the field is absent or outside 0 .. 2^32 - 2    */
  uint32_t *key_id;
  int64_t *ts;                /* max of the two records' timestamps             */
  void *const *cols;          /* n_cols[0] + n_cols[1] arrays: this side's
                                 columns, then the other side's                 */
  uint8_t *const *valid;      /* optional; each entry may be NULL               */
  uint64_t *this_handle;      /* optional                                       */
  uint64_t *other_handle;     /* optional                                       */
  uint32_t *join_key;         /* optional                                       */
} hsg_join_joined;

int  hsg_join_create_valued(hsg_engine *eng, const hsg_join_config *cfg, const hsg_join_values *vals,
                            hsg_join **out);
/* batch->handle is ignored and may be NULL. hsg_join_push on a valued join and
 * hsg_join_push_valued on a plain one return HSG_E_INVALID. */
int  hsg_join_push_valued(hsg_join *j, const hsg_join_batch *batch, const hsg_join_cols *cols);
/* hsg_join_drain's capacity rule: capacity < pending returns HSG_E_CAPACITY,
 * sets *n_out = pending and consumes nothing. The arrays are complete when the
 * call returns (they can go into hsg_push_batch with no event). On a plain
 * join: HSG_E_INVALID. */
int  hsg_join_drain_batch(hsg_join *j, hsg_join_joined *out, uint64_t *n_out);
/* value rows in use (records pushed) and allocated */
int  hsg_join_value_rows(const hsg_join *j, uint64_t *used, uint64_t *capacity);
/* 8-byte words per value row for sides of c0 and c1 columns: the smallest
 * power of two >= max(c0, c1) + 1 (values, then one word of valid bytes);
 * 0 for counts a valued join refuses */
uint64_t hsg_join_value_stride(int32_t c0, int32_t c1);

#ifdef __cplusplus
}
#endif

#endif /* HSTREAM_JOIN_H */
