// Internal entry points between the orchestration files. Not part of the ABI.
#pragma once

#include <string>

#include "hsg_internal.h"
#include "hsg_ops.h"

namespace hsg {

// op_device.cpp
int stage_batch(OpDevice &d, const hsg_batch *b, Batch &kb, std::string &err, int staged_set = -1);
TwParams make_tw_params(const hsg_op_config &cfg, const PushArgs &a);
void launch_stream_time(OpDevice &d, const hsg_op_config &cfg, const Batch &kb, int64_t wm_in, int64_t adv);
int fetch_scalars(OpDevice &d, std::string &err);
// wait for stream s: poll an event (5 ms), then block
int poll_stream(OpDevice &d, hipStream_t s, std::string &err);
int clear_batch_scalars(OpDevice &d, std::string &err);
int finish_batch(OpDevice &d, int64_t wm_in, uint64_t n, PushResult &r, std::string &err);
int push_local(OpDevice &d, const hsg_op_config &cfg, const Program &prog, const PushArgs &a, const Batch &kb,
               const int64_t *seq, const int64_t *rec_wm, PushResult &r, std::string &err);

// per-record changelog for time windows (perrecord.cpp / k_perrecord.hip)
int perrecord_device_init(OpDevice &d, const hsg_op_config &cfg, const Program &prog, std::string &err);
int part_device_init(OpDevice &d, const hsg_op_config &cfg, const Program &prog, std::string &err);
bool perrecord_part_eligible(const Program &prog, uint64_t wpr);
int perrecord_part_init(OpDevice &d, const hsg_op_config &cfg, const Program &prog, std::string &err);
int push_time_perrecord(OpDevice &d, const hsg_op_config &cfg, const Program &prog, const PushArgs &a,
                        const Batch &kb, const int64_t *seq, const int64_t *rec_wm, PushResult &r, std::string &err);

// sessions (session.cpp / k_session.hip)
int session_device_init(OpDevice &d, const hsg_op_config &cfg, const Program &prog, uint64_t rows, std::string &err);
int session_device_reset(OpDevice &d, std::string &err);
void session_device_free(OpDevice &d);
int push_session(OpDevice &d, const hsg_op_config &cfg, const Program &prog, const PushArgs &a, const Batch &kb,
                 const int64_t *seq, PushResult &r, std::string &err);
void launch_session_dump(OpDevice &d, const hsg_op_config &cfg, const Program &prog, OutCols out, uint64_t cap,
                         uint64_t *counter);

// keyed view reads (hsg_view_get: op_device.cpp op_view_get / k_view.hip).
// Every launcher takes the request's keys sorted ascending, distinct, without
// HSG_KEY_NONE, in device memory (nk <= HSG_VIEW_MAX_KEYS).
//
// Time windows: the slots scanned are the distinct key-hash regions of the
// requested keys (tw_region_base) and the overflow rows, cut into chunks of
// kEmitChunk slots, one workgroup each: chunks [0, n_regions * cpr) cover the
// regions in the order of `region`, the rest the overflow rows.
struct ViewScan {
  const uint64_t *region;  // device: first slot of each distinct region, ascending
  uint32_t n_regions;
  uint32_t cpr;            // chunks per region
  uint64_t rslots;         // slots per region
  uint64_t ovf_base;       // first overflow row (0 slots: none scanned)
  uint64_t ovf_slots;
  uint64_t chunks() const { return (uint64_t)n_regions * cpr + (ovf_slots + kEmitChunk - 1) / kEmitChunk; }
};
// chunk counts -> es.cnt, their exclusive scan -> es.off, the total -> *total (device)
void launch_view_tw_count(hipStream_t s, const TwTable &t, const ViewScan &v, const uint32_t *keys, uint32_t nk,
                          const EmitScratch &es, uint64_t *total);
// the counted rows, rendered, at out[es.off[chunk] ...] in scan order
void launch_view_tw_rows(hipStream_t s, const TwTable &t, const ViewScan &v, const uint32_t *keys, uint32_t nk,
                         const Program &prog, const TwParams &p, const EmitScratch &es, OutCols out, uint64_t out_cap,
                         DevScalars *sc);
// Unwindowed ops and sessions: one lookup per key (tw_find / ss_find) leaves
// the key's table slot (-1: absent) and its row count; one workgroup scans the
// counts into row offsets (off[nk] = the total); the rows come out in key order.
void launch_view_kv_find(hipStream_t s, const TwTable &t, const uint32_t *keys, uint32_t nk, int64_t *slot,
                         uint32_t *cnt);
void launch_view_ss_find(hipStream_t s, const SessTable &t, const uint32_t *keys, uint32_t nk, int64_t *slot,
                         uint32_t *cnt);
void launch_view_scan(hipStream_t s, const uint32_t *cnt, uint32_t nk, uint64_t *off);
void launch_view_kv_rows(hipStream_t s, const TwTable &t, const Program &prog, const uint32_t *keys, uint32_t nk,
                         const int64_t *slot, const uint64_t *off, OutCols out, uint64_t out_cap);
void launch_view_ss_rows(hipStream_t s, const SessTable &t, const Program &prog, const uint32_t *keys, uint32_t nk,
                         const int64_t *slot, const uint64_t *off, OutCols out, uint64_t out_cap);

// stream-table join (hsg_table_join: op_device.cpp op_table_join / k_tjoin.hip).
// The probe batch's keys (device memory, arrival order, HSG_KEY_NONE allowed)
// are cut into tiles of kTjTile records, one workgroup each.
constexpr uint64_t kTjTile = 1024;
inline uint64_t tjoin_tiles(uint64_t n) { return (n + kTjTile - 1) / kTjTile; }
// each record's table slot (-1: no live row) -> slot[n]; the tiles' hit counts
// -> es.cnt, their exclusive scan -> es.off, the total -> *total (device)
void launch_tjoin_find(hipStream_t s, const TwTable &t, const uint32_t *keys, uint64_t n, int64_t *slot,
                       const EmitScratch &es, uint64_t *total);
// the hits' rows, rendered, in arrival order at out[0 .. total); null columns
// of out are skipped
void launch_tjoin_rows(hipStream_t s, const TwTable &t, const Program &prog, const uint32_t *keys, uint64_t n,
                       const int64_t *slot, const EmitScratch &es, OutCols out, uint64_t out_cap);

// multi-GPU key exchange (exchange.cpp / k_exchange.hip)
int exchange_device_init(OpDevice &d, const hsg_op_config &cfg, uint64_t batch_cap, std::string &err);
void exchange_device_free(OpDevice &d);
int push_sharded(OpDevice &d, const hsg_op_config &cfg, const Program &prog, const PushArgs &a, PushResult &r,
                 std::string &err);

}  // namespace hsg
