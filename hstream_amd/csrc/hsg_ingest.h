// Device JSON ingest (include/hstream_ingest.h hsg_gpu_decode_json): what
// gpu_ingest.cpp hands k_ingest.hip. Not part of the ABI.
#pragma once

#include "hsg_internal.h"
#include "hsg_json.h"

namespace hsg {

// the decode kernel's DevScalars::err bit (the look-back gave up)
constexpr uint32_t ERR_INGEST = 16u;
// records per tile, one per thread
constexpr int kIngestTile = 256;
// LDS bytes a tile's records are staged in; a longer tile is scanned from HBM
constexpr uint32_t kIngestLds = 32768;
// DevScalars::scratch word the last tile leaves kIngestRan | fallback count in
constexpr int kIngestWord = 0;
constexpr uint64_t kIngestRan = 1ull << 61;

struct IngestArgs {
  uint64_t n;
  const uint8_t *buf;      // the batch's bytes, buf[0] = byte off[0] of the caller's buffer; 16-byte
                           // aligned and readable up to the next multiple of 16 past the last byte
  const uint64_t *off;     // n + 1 offsets, ascending (checked by the host)
  const jf::Targets *tg;
  const jf::KeyEntry *table;
  uint64_t table_mask;     // slots - 1
  uint32_t *key_id;
  int64_t *col[kMaxCols];
  uint8_t *valid[kMaxCols];
  uint32_t *spell;         // null: spellings not asked for
  uint32_t *list;          // the fallback records' indices, ascending
  uint64_t *state;         // [0] tile tickets, [2 ..] one word per tile; zeroed before the launch
  DevScalars *sc;
};

struct IngestPatch {
  uint64_t cnt;
  int32_t n_cols;
  const uint32_t *list;
  // the host decoder's rows of the listed records, row j = record list[j]
  const uint32_t *h_key, *h_spell;
  const int64_t *h_col[kMaxCols];
  const uint8_t *h_valid[kMaxCols];
  uint32_t *key_id;
  int64_t *col[kMaxCols];
  uint8_t *valid[kMaxCols];
  uint32_t *spell;
};

void launch_json_decode(hipStream_t s, int n_cols, const IngestArgs &a);
void launch_ingest_patch(hipStream_t s, const IngestPatch &a);
// ents[j] -> table[slot[j]] (the host picked the slots: it keeps the table's mirror)
void launch_ingest_table_put(hipStream_t s, jf::KeyEntry *table, const uint64_t *slot, const jf::KeyEntry *ents,
                             uint64_t n);

}  // namespace hsg
