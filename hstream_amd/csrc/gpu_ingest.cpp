// Host runtime of the device JSON ingest (include/hstream_ingest.h
// hsg_gpu_decode_json): upload a poll batch's bytes, run k_json_decode
// (k_ingest.hip), read the fallback list back, send those records through the
// unchanged host decoder in record order, patch their rows in, and keep the
// device key table level with the dictionary.
//
// The key table is built on the host: the decoder keeps a mirror of it, picks
// the slot of every new entry there (linear probing, load <= 1/2), and
// k_ingest_table_put writes the new entries at those slots; a table that has
// to grow is rebuilt in the mirror at twice the slots and uploaded whole. No
// kernel inserts, so the decode kernel reads a table nothing else writes.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/hstream_ingest.h"
#include "hsg_ingest.h"

using namespace hsg;

namespace hsg {
// hsg_api.cpp
int engine_device(const hsg_engine *e);
// ingest.cpp: the keys' canonical bytes and first-spelling forms, id after id
void keydict_canon(const hsg_keydict *d, const char **canon, const uint64_t **coff, const char **form,
                   const uint64_t **foff, uint64_t *n);
}  // namespace hsg

namespace {

// records of the fallback list that travel with the call's one device-to-host
// read; a longer list costs a second read
constexpr uint64_t kHeadList = 4096;

struct OutSet {
  uint32_t *key = nullptr, *spell = nullptr;
  int64_t *ts = nullptr;
  int64_t *col[kMaxCols] = {};
  uint8_t *valid[kMaxCols] = {};
  hipEvent_t ev = nullptr;
  const void *colp[kMaxCols] = {};
  const uint8_t *validp[kMaxCols] = {};
};

bool subset_bytes(const char *s, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    const uint8_t c = (uint8_t)s[i];
    if (c < 0x20 || c > 0x7E || c == '"' || c == '\\') return false;
  }
  return true;
}

// The decoder configuration as the scanner takes it; false: outside the
// device path's limits (the caller keeps the host decoder).
bool make_targets(const hsg_decoder_config *cfg, jf::Targets &t) {
  memset(&t, 0, sizeof(t));
  if (!cfg || cfg->n_cols < 0 || cfg->n_cols > jf::kMaxCols) return false;
  if (cfg->n_cols && (!cfg->col_fields || !cfg->col_types)) return false;
  auto put = [&](int k, const char *s) {
    const size_t n = strlen(s);
    if (n > jf::kMaxName || !subset_bytes(s, n)) return false;
    memcpy(t.name[k], s, n);
    t.len[k] = (uint8_t)n;
    return true;
  };
  t.keyless = cfg->key_field ? 0 : 1;
  if (cfg->key_field && !put(0, cfg->key_field)) return false;
  t.literal_forms = cfg->literal_forms ? 1 : 0;
  t.n_cols = (uint8_t)cfg->n_cols;
  for (int c = 0; c < cfg->n_cols; ++c) {
    if (!cfg->col_fields[c] || !put(c + 1, cfg->col_fields[c])) return false;
    if (cfg->col_types[c] == HSG_F64) t.f64_mask |= (uint8_t)(1u << c);
    else if (cfg->col_types[c] != HSG_I64) return false;
    if (!cfg->col_numeric || cfg->col_numeric[c]) t.num_mask |= (uint8_t)(1u << c);
  }
  return true;
}

// A key's canonical bytes (ingest.cpp: z | t | f | n0 | n<+|-><digits>e<exp>; |
// s<u32 len><utf8> | [..] | {..}) as a table entry; false: a key the subset
// cannot express, which stays with the host.
bool entry_of(const char *c, size_t n, const char *form, size_t fn, uint32_t id, jf::KeyEntry &e) {
  memset(&e, 0, sizeof(e));
  e.id1 = id + 1;
  if (!n) return false;
  if (n == 1 && (c[0] == 'z' || c[0] == 't' || c[0] == 'f')) {
    e.tag = (uint8_t)c[0];
  } else if (c[0] == 'n') {
    e.tag = 'n';
    e.len = 13;
    e.form = fn == 1 ? (uint8_t)form[0] : 0;
    if (!(n == 2 && c[1] == '0')) {
      if (n < 5 || (c[1] != '+' && c[1] != '-')) return false;
      size_t i = 2;
      uint64_t m = 0;
      size_t nd = 0;
      while (i < n && c[i] >= '0' && c[i] <= '9') {
        if (++nd > jf::kMaxDigits) return false;
        m = m * 10 + (uint64_t)(c[i] - '0');
        ++i;
      }
      if (!nd || i >= n || c[i] != 'e') return false;
      ++i;
      bool eneg = false;
      if (i < n && c[i] == '-') eneg = true, ++i;
      int64_t ex = 0;
      size_t ne = 0;
      while (i < n && c[i] >= '0' && c[i] <= '9') {
        if (++ne > 9) return false;
        ex = ex * 10 + (c[i] - '0');
        ++i;
      }
      if (!ne || i + 1 != n || c[i] != ';') return false;
      if (eneg) ex = -ex;
      e.w[0] = m;
      e.w[1] = (uint64_t)(uint32_t)(int32_t)ex | ((uint64_t)(c[1] == '-') << 32);
    }
  } else if (c[0] == 's') {
    if (n < 5) return false;
    uint32_t len;
    memcpy(&len, c + 1, 4);
    if ((size_t)len + 5 != n || len > jf::kMaxKey || !subset_bytes(c + 5, len)) return false;
    e.tag = 's';
    e.len = (uint8_t)len;
    memcpy(e.w, c + 5, len);
  } else {
    return false;
  }
  e.hash = jf::key_hash(e.tag, e.len, e.w);
  return true;
}

}  // namespace

struct hsg_gpu_decoder {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  hsg_decoder *host = nullptr;
  hsg_keydict *dict = nullptr;
  jf::Targets tg;
  int C = 0;
  uint64_t max_records = 0, max_bytes = 0;
  // inputs
  uint8_t *d_buf = nullptr;
  uint64_t *d_off = nullptr;
  jf::Targets *d_tg = nullptr;
  uint8_t *d_head = nullptr;   // DevScalars, then the fallback list (max_records entries)
  uint64_t *d_state = nullptr;
  uint8_t *h_head = nullptr;   // pinned: DevScalars + kHeadList entries
  OutSet out[2];
  int next = 0;
  // the fallback records' host rows, and their device copies
  std::vector<uint32_t> list, h_key, h_spell;
  std::vector<int64_t> h_col[kMaxCols];
  std::vector<uint8_t> h_valid[kMaxCols], h_status;
  std::vector<char> tmp;
  std::vector<uint64_t> toff;
  uint32_t *p_key = nullptr, *p_spell = nullptr;
  int64_t *p_col[kMaxCols] = {};
  uint8_t *p_valid[kMaxCols] = {};
  // key table
  std::vector<jf::KeyEntry> mirror;
  jf::KeyEntry *d_table = nullptr;
  uint64_t used = 0, synced = 0, rebuilds = 0;
  std::vector<uint64_t> put_slot;
  std::vector<jf::KeyEntry> put_ent;
  uint64_t *d_put_slot = nullptr;
  jf::KeyEntry *d_put_ent = nullptr;
  uint64_t put_cap = 0;
};

namespace {

#define GTRY(expr)                                                          \
  do {                                                                      \
    hipError_t _e = (expr);                                                 \
    if (_e != hipSuccess) {                                                 \
      g->err = std::string(#expr) + ": " + hipGetErrorString(_e);           \
      return _e == hipErrorOutOfMemory ? HSG_E_OOM : HSG_E_DEVICE;          \
    }                                                                       \
  } while (0)

template <typename T>
hipError_t dmalloc(T *&p, uint64_t count) {
  return hipMalloc((void **)&p, (count ? count : 1) * sizeof(T));
}
void dfree(void *p) {
  if (p) hipFree(p);
}

void free_decoder(hsg_gpu_decoder *g) {
  if (!g) return;
  hipSetDevice(g->device);
  if (g->stream) hipStreamSynchronize(g->stream);
  for (OutSet &o : g->out) {
    dfree(o.key);
    dfree(o.spell);
    dfree(o.ts);
    for (int c = 0; c < kMaxCols; ++c) dfree(o.col[c]), dfree(o.valid[c]);
    if (o.ev) hipEventDestroy(o.ev);
  }
  void *ptrs[] = {g->d_buf, g->d_off, g->d_tg, g->d_head, g->d_state, g->p_key, g->p_spell, g->d_table,
                  g->d_put_slot, g->d_put_ent};
  for (void *p : ptrs) dfree(p);
  for (int c = 0; c < kMaxCols; ++c) dfree(g->p_col[c]), dfree(g->p_valid[c]);
  if (g->h_head) hipHostFree(g->h_head);
  if (g->stream) hipStreamDestroy(g->stream);
  if (g->host) hsg_decoder_destroy(g->host);
  delete g;
}

// slot of a new entry in the mirror (its key is not there)
uint64_t mirror_slot(const std::vector<jf::KeyEntry> &m, uint64_t h) {
  const uint64_t mask = m.size() - 1;
  uint64_t q = h & mask;
  while (m[q].id1) q = (q + 1) & mask;
  return q;
}

// Bring the device table level with the dictionary: the ids added since the
// last sync, whoever added them.
int sync_table(hsg_gpu_decoder *g) {
  if (g->tg.keyless || !g->dict) return HSG_OK;
  const char *canon, *form;
  const uint64_t *coff, *foff;
  uint64_t nk;
  keydict_canon(g->dict, &canon, &coff, &form, &foff, &nk);
  if (nk <= g->synced) return HSG_OK;
  g->put_slot.clear();
  g->put_ent.clear();
  std::vector<jf::KeyEntry> fresh;
  for (uint64_t id = g->synced; id < nk; ++id) {
    jf::KeyEntry e;
    if (entry_of(canon + coff[id], (size_t)(coff[id + 1] - coff[id]), form + foff[id],
                 (size_t)(foff[id + 1] - foff[id]), (uint32_t)id, e))
      fresh.push_back(e);
  }
  // synced advances only once the device table holds the entries: a failed
  // upload leaves the ids to the next call's sync
  if (fresh.empty()) {
    g->synced = nk;
    return HSG_OK;
  }
  uint64_t slots = g->mirror.size();
  while (2 * (g->used + fresh.size()) > slots) slots *= 2;
  if (slots != g->mirror.size()) {
    // grow by rebuild: every entry again, at twice the slots (or more), uploaded whole
    std::vector<jf::KeyEntry> m(slots);
    memset(m.data(), 0, slots * sizeof(jf::KeyEntry));
    for (const jf::KeyEntry &e : g->mirror)
      if (e.id1) m[mirror_slot(m, e.hash)] = e;
    for (const jf::KeyEntry &e : fresh) m[mirror_slot(m, e.hash)] = e;
    jf::KeyEntry *nt = nullptr;
    GTRY(dmalloc(nt, slots));
    hipError_t e1 = hipMemcpyAsync(nt, m.data(), slots * sizeof(jf::KeyEntry), hipMemcpyHostToDevice, g->stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(g->stream);
    if (e1 != hipSuccess) {
      hipFree(nt);
      g->err = std::string("key table upload: ") + hipGetErrorString(e1);
      return HSG_E_DEVICE;
    }
    dfree(g->d_table);
    g->d_table = nt;
    g->mirror.swap(m);
    g->used += fresh.size();
    g->synced = nk;
    ++g->rebuilds;
    return HSG_OK;
  }
  const uint64_t np = fresh.size();
  if (np > g->put_cap) {
    // (the stream may still read the old staging: hipFree waits for it)
    dfree(g->d_put_slot);
    dfree(g->d_put_ent);
    g->d_put_slot = nullptr;
    g->d_put_ent = nullptr;
    g->put_cap = 0;
    const uint64_t cap = np < 1024 ? 1024 : 2 * np;
    GTRY(dmalloc(g->d_put_slot, cap));
    GTRY(dmalloc(g->d_put_ent, cap));
    g->put_cap = cap;
  }
  for (const jf::KeyEntry &e : fresh) {
    const uint64_t q = mirror_slot(g->mirror, e.hash);
    g->mirror[q] = e;
    g->put_slot.push_back(q);
    g->put_ent.push_back(e);
  }
  hipError_t e1 = hipMemcpyAsync(g->d_put_slot, g->put_slot.data(), np * 8, hipMemcpyHostToDevice, g->stream);
  if (e1 == hipSuccess)
    e1 = hipMemcpyAsync(g->d_put_ent, g->put_ent.data(), np * sizeof(jf::KeyEntry), hipMemcpyHostToDevice, g->stream);
  if (e1 == hipSuccess) {
    launch_ingest_table_put(g->stream, g->d_table, g->d_put_slot, g->d_put_ent, np);
    e1 = hipGetLastError();
  }
  // the staging vectors are rewritten by the next sync
  if (e1 == hipSuccess) e1 = hipStreamSynchronize(g->stream);
  if (e1 != hipSuccess) {
    for (uint64_t q : g->put_slot) g->mirror[q].id1 = 0;  // not in the device table: retried by the next sync
    g->err = std::string("key table update: ") + hipGetErrorString(e1);
    return HSG_E_DEVICE;
  }
  g->used += np;
  g->synced = nk;
  return HSG_OK;
}

int create_impl(hsg_gpu_decoder *g, hsg_engine *eng, const hsg_decoder_config *cfg, uint64_t table_slots0) {
  g->device = engine_device(eng);
  GTRY(hipSetDevice(g->device));
  GTRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking));
  const uint64_t nr = g->max_records, C = (uint64_t)g->C;
  GTRY(dmalloc(g->d_buf, g->max_bytes + 32));
  GTRY(dmalloc(g->d_off, nr + 1));
  GTRY(dmalloc(g->d_tg, 1));
  GTRY(dmalloc(g->d_head, sizeof(DevScalars) + 4 * nr));
  GTRY(dmalloc(g->d_state, 2 + (nr + kIngestTile - 1) / kIngestTile));
  GTRY(hipHostMalloc((void **)&g->h_head, sizeof(DevScalars) + 4 * kHeadList, hipHostMallocDefault));
  for (OutSet &o : g->out) {
    GTRY(dmalloc(o.key, nr));
    GTRY(dmalloc(o.spell, nr));
    GTRY(dmalloc(o.ts, nr));
    for (uint64_t c = 0; c < C; ++c) {
      GTRY(dmalloc(o.col[c], nr));
      GTRY(dmalloc(o.valid[c], nr));
      o.colp[c] = o.col[c];
      o.validp[c] = o.valid[c];
    }
    GTRY(hipEventCreateWithFlags(&o.ev, hipEventDisableTiming));
  }
  GTRY(dmalloc(g->p_key, nr));
  GTRY(dmalloc(g->p_spell, nr));
  for (uint64_t c = 0; c < C; ++c) {
    GTRY(dmalloc(g->p_col[c], nr));
    GTRY(dmalloc(g->p_valid[c], nr));
  }
  GTRY(hipMemcpyAsync(g->d_tg, &g->tg, sizeof(jf::Targets), hipMemcpyHostToDevice, g->stream));
  uint64_t slots = 64;
  while (slots < table_slots0 && slots < (1ull << 40)) slots *= 2;
  g->mirror.resize(slots);
  memset(g->mirror.data(), 0, slots * sizeof(jf::KeyEntry));
  GTRY(dmalloc(g->d_table, slots));
  GTRY(hipMemsetAsync(g->d_table, 0, slots * sizeof(jf::KeyEntry), g->stream));
  GTRY(hipStreamSynchronize(g->stream));
  int rc = hsg_decoder_create(cfg, &g->host);
  if (rc != HSG_OK) return rc;
  return HSG_OK;
}

int decode_impl(hsg_gpu_decoder *g, uint64_t n, const char *buf, const uint64_t *off, const int64_t *rec_ts,
                hsg_batch *out, uint8_t *status, uint64_t *rejected, int want_spell, hsg_sink_spellings *spell_out,
                hsg_gpu_decode_stats *stats, int n_threads) {
  const int C = g->C;
  GTRY(hipSetDevice(g->device));
  const uint64_t keys0 = g->dict ? hsg_keydict_size(g->dict) : 0;
  int rc = sync_table(g);
  if (rc != HSG_OK) return rc;
  OutSet &o = g->out[g->next];
  uint64_t cnt = 0;
  if (rejected) *rejected = 0;
  if (n) {
    const uint64_t bytes = off[n] - off[0];
    if (bytes) GTRY(hipMemcpyAsync(g->d_buf, buf + off[0], bytes, hipMemcpyHostToDevice, g->stream));
    GTRY(hipMemcpyAsync(g->d_off, off, (n + 1) * 8, hipMemcpyHostToDevice, g->stream));
    if (rec_ts) GTRY(hipMemcpyAsync(o.ts, rec_ts, n * 8, hipMemcpyHostToDevice, g->stream));
    else GTRY(hipMemsetAsync(o.ts, 0, n * 8, g->stream));
    const uint64_t tiles = (n + kIngestTile - 1) / kIngestTile;
    GTRY(hipMemsetAsync(g->d_state, 0, (2 + tiles) * 8, g->stream));
    GTRY(hipMemsetAsync(g->d_head, 0, sizeof(DevScalars), g->stream));
    IngestArgs a = {};
    a.n = n;
    a.buf = g->d_buf;
    a.off = g->d_off;
    a.tg = g->d_tg;
    a.table = g->d_table;
    a.table_mask = g->mirror.size() - 1;
    a.key_id = o.key;
    for (int c = 0; c < C; ++c) a.col[c] = o.col[c], a.valid[c] = o.valid[c];
    a.spell = want_spell ? o.spell : nullptr;
    a.list = reinterpret_cast<uint32_t *>(g->d_head + sizeof(DevScalars));
    a.state = g->d_state;
    a.sc = reinterpret_cast<DevScalars *>(g->d_head);
    launch_json_decode(g->stream, C, a);
    GTRY(hipGetLastError());
    // the call's one device-to-host read: the scalars and the head of the list
    const uint64_t head = n < kHeadList ? n : kHeadList;
    GTRY(hipMemcpyAsync(g->h_head, g->d_head, sizeof(DevScalars) + 4 * head, hipMemcpyDeviceToHost, g->stream));
    GTRY(hipStreamSynchronize(g->stream));
    const DevScalars *sc = reinterpret_cast<const DevScalars *>(g->h_head);
    const uint64_t word = sc->scratch[kIngestWord];
    if ((sc->err & ERR_INGEST) || !(word & kIngestRan)) {
      g->err = "device JSON decode did not complete";
      return HSG_E_DEVICE;
    }
    cnt = word & ~kIngestRan;
    if (cnt > n) {
      g->err = "device JSON decode: fallback count out of range";
      return HSG_E_DEVICE;
    }
    g->list.resize(cnt);
    const uint64_t got = cnt < head ? cnt : head;
    if (got) memcpy(g->list.data(), g->h_head + sizeof(DevScalars), 4 * got);
    if (cnt > got)  // a long list (a batch of new keys): the rest in a second read
      GTRY(hipMemcpy(g->list.data() + got, g->d_head + sizeof(DevScalars) + 4 * got, 4 * (cnt - got),
                     hipMemcpyDeviceToHost));
  }
  if (status && n) memset(status, HSG_DEC_OK, n);
  if (cnt) {
    // the fallback records, back to back, through the host decoder in record order
    uint64_t tb = 0;
    for (uint64_t j = 0; j < cnt; ++j) {
      const uint64_t i = g->list[j];
      if (i >= n || (j && i <= g->list[j - 1])) {
        g->err = "device JSON decode: fallback list out of order";
        return HSG_E_DEVICE;
      }
      tb += off[i + 1] - off[i];
    }
    g->tmp.resize(tb ? tb : 1);
    g->toff.resize(cnt + 1);
    tb = 0;
    for (uint64_t j = 0; j < cnt; ++j) {
      const uint64_t i = g->list[j], len = off[i + 1] - off[i];
      g->toff[j] = tb;
      if (len) memcpy(g->tmp.data() + tb, buf + off[i], len);
      tb += len;
    }
    g->toff[cnt] = tb;
    g->h_key.resize(cnt);
    g->h_spell.resize(cnt);
    g->h_status.resize(cnt);
    void *cp[kMaxCols] = {};
    uint8_t *vp[kMaxCols] = {};
    for (int c = 0; c < C; ++c) {
      g->h_col[c].resize(cnt);
      g->h_valid[c].resize(cnt);
      cp[c] = g->h_col[c].data();
      vp[c] = g->h_valid[c].data();
    }
    uint64_t rej = 0;
    rc = hsg_decode_json_spelled(g->host, g->dict, cnt, g->tmp.data(), g->toff.data(), nullptr, g->h_key.data(),
                                 nullptr, cp, vp, g->h_status.data(), &rej, want_spell ? g->h_spell.data() : nullptr,
                                 n_threads);
    if (rc != HSG_OK) {
      g->err = "host decoder failed on the fallback records";
      return rc;
    }
    if (rejected) *rejected = rej;
    if (status)
      for (uint64_t j = 0; j < cnt; ++j) status[g->list[j]] = g->h_status[j];
    // their rows over the kernel's
    GTRY(hipMemcpyAsync(g->p_key, g->h_key.data(), 4 * cnt, hipMemcpyHostToDevice, g->stream));
    if (want_spell) GTRY(hipMemcpyAsync(g->p_spell, g->h_spell.data(), 4 * cnt, hipMemcpyHostToDevice, g->stream));
    for (int c = 0; c < C; ++c) {
      GTRY(hipMemcpyAsync(g->p_col[c], g->h_col[c].data(), 8 * cnt, hipMemcpyHostToDevice, g->stream));
      GTRY(hipMemcpyAsync(g->p_valid[c], g->h_valid[c].data(), cnt, hipMemcpyHostToDevice, g->stream));
    }
    IngestPatch p = {};
    p.cnt = cnt;
    p.n_cols = C;
    p.list = reinterpret_cast<const uint32_t *>(g->d_head + sizeof(DevScalars));
    p.h_key = g->p_key;
    p.h_spell = g->p_spell;
    p.key_id = o.key;
    p.spell = want_spell ? o.spell : nullptr;
    for (int c = 0; c < C; ++c) {
      p.h_col[c] = g->p_col[c];
      p.h_valid[c] = g->p_valid[c];
      p.col[c] = o.col[c];
      p.valid[c] = o.valid[c];
    }
    launch_ingest_patch(g->stream, p);
    GTRY(hipGetLastError());
    // the host vectors are rewritten by the next call
    GTRY(hipStreamSynchronize(g->stream));
    rc = sync_table(g);
    if (rc != HSG_OK) return rc;
  }
  GTRY(hipEventRecord(o.ev, g->stream));
  memset(out, 0, sizeof(*out));
  out->n = n;
  out->mem = HSG_MEM_DEVICE;
  out->n_cols = C;
  out->key_id = o.key;
  out->ts = o.ts;
  out->cols = o.colp;
  out->valid = o.validp;
  out->ready_event = o.ev;
  if (spell_out) {
    memset(spell_out, 0, sizeof(*spell_out));
    if (want_spell) {
      spell_out->spell = o.spell;
      spell_out->n = n;
      spell_out->mem = HSG_MEM_DEVICE;
    }
  }
  if (stats) {
    stats->records = n;
    stats->accepted = n - cnt;
    stats->host_records = cnt;
    stats->new_keys = (g->dict ? hsg_keydict_size(g->dict) : 0) - keys0;
    stats->table_slots = g->mirror.size();
    stats->table_rebuilds = g->rebuilds;
  }
  g->next ^= 1;
  return HSG_OK;
}

}  // namespace

extern "C" int hsg_gpu_decoder_create(hsg_engine *eng, const hsg_decoder_config *cfg, hsg_keydict *dict,
                                      uint64_t max_records, uint64_t max_bytes, uint64_t table_slots0,
                                      hsg_gpu_decoder **out) {
  if (!eng || !cfg || !out) return HSG_E_INVALID;
  *out = nullptr;
  if (!max_records || max_records >= (1ull << 32) || (cfg->key_field && !dict)) return HSG_E_INVALID;
  hsg_gpu_decoder *g = nullptr;
  try {
    g = new hsg_gpu_decoder();
    if (!make_targets(cfg, g->tg)) {
      delete g;
      return HSG_E_INVALID;
    }
    g->C = cfg->n_cols;
    g->dict = cfg->key_field ? dict : nullptr;
    g->max_records = max_records;
    g->max_bytes = max_bytes;
    const int rc = create_impl(g, eng, cfg, table_slots0);
    if (rc != HSG_OK) {
      free_decoder(g);
      return rc;
    }
    *out = g;
    return HSG_OK;
  } catch (const std::bad_alloc &) {
    free_decoder(g);
    return HSG_E_OOM;
  } catch (...) {
    free_decoder(g);
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_gpu_decode_json(hsg_gpu_decoder *g, uint64_t n, const char *buf, const uint64_t *off,
                                   const int64_t *rec_ts, hsg_batch *out, uint8_t *status, uint64_t *rejected,
                                   int want_spell, hsg_sink_spellings *spell_out, hsg_gpu_decode_stats *stats,
                                   int n_threads) {
  if (!g || !out || (n && (!buf || !off))) return HSG_E_INVALID;
  if (n > g->max_records) return HSG_E_CAPACITY;
  for (uint64_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return HSG_E_INVALID;
  if (n && off[n] - off[0] > g->max_bytes) return HSG_E_CAPACITY;
  try {
    return decode_impl(g, n, buf, off, rec_ts, out, status, rejected, want_spell, spell_out, stats, n_threads);
  } catch (const std::bad_alloc &) {
    return HSG_E_OOM;
  } catch (...) {
    return HSG_E_DEVICE;
  }
}

extern "C" int hsg_gpu_decoder_fetch(hsg_gpu_decoder *g, const hsg_batch *b, const hsg_sink_spellings *sp,
                                     uint32_t *key_id, int64_t *ts, void *const *cols, uint8_t *const *valid,
                                     uint32_t *spell) {
  if (!g || !b || b->mem != HSG_MEM_DEVICE || b->n_cols != g->C) return HSG_E_INVALID;
  GTRY(hipSetDevice(g->device));
  if (b->ready_event) GTRY(hipEventSynchronize((hipEvent_t)b->ready_event));
  const uint64_t n = b->n;
  if (!n) return HSG_OK;
  if (key_id) GTRY(hipMemcpy(key_id, b->key_id, 4 * n, hipMemcpyDeviceToHost));
  if (ts) GTRY(hipMemcpy(ts, b->ts, 8 * n, hipMemcpyDeviceToHost));
  for (int c = 0; c < g->C; ++c) {
    if (cols && cols[c]) GTRY(hipMemcpy(cols[c], b->cols[c], 8 * n, hipMemcpyDeviceToHost));
    if (valid && valid[c]) GTRY(hipMemcpy(valid[c], b->valid[c], n, hipMemcpyDeviceToHost));
  }
  if (spell && sp && sp->spell && sp->n == n) GTRY(hipMemcpy(spell, sp->spell, 4 * n, hipMemcpyDeviceToHost));
  return HSG_OK;
}

extern "C" void hsg_gpu_decoder_destroy(hsg_gpu_decoder *g) { free_decoder(g); }

extern "C" const char *hsg_gpu_decoder_last_error(const hsg_gpu_decoder *g) { return g ? g->err.c_str() : ""; }

extern "C" int hsg_json_fast_probe(const hsg_decoder_config *cfg, const char *rec, uint64_t len, hsg_json_probe *out) {
  if (!cfg || !out || (len && !rec)) return HSG_E_INVALID;
  jf::Targets t;
  if (!make_targets(cfg, t)) return HSG_E_INVALID;
  memset(out, 0, sizeof(*out));
  if (len > jf::kMaxRecord) return HSG_OK;
  jf::Scan r;
  jf::scan_record<jf::kMaxCols>(reinterpret_cast<const uint8_t *>(rec), (uint32_t)len, t, r);
  out->accept = (int32_t)r.accept;
  out->key_tag = r.key_tag;
  out->key_neg = r.key_neg;
  out->key_int_form = r.key_iform;
  out->key_e = r.key_e;
  out->key_m = r.key_m;
  out->key_off = r.key_off;
  out->key_len = r.key_len;
  if (r.accept)
    for (int c = 0; c < jf::kMaxCols; ++c) {
      out->words[c] = r.word[c];
      out->valid[c] = r.valid[c];
    }
  return HSG_OK;
}
