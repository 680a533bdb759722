// Device JSON ingest: a poll batch's record bytes into the columns of an
// hsg_batch (include/hstream_ingest.h hsg_gpu_decode_json).
//
// k_json_decode<C>: a workgroup takes tiles of kIngestTile consecutive records
// (hsg_lookback.h: tickets in order). A tile's bytes are contiguous in the
// batch, [off[r0], off[r1]); widened to 16-byte bounds they are copied into
// LDS with coalesced 16-byte loads, and each lane scans its own record from
// LDS with the scanner of hsg_json.h. A tile whose bytes exceed the LDS buffer
// is scanned from HBM instead: the same answers, uncoalesced byte loads.
// An accepted record probes the key table (linear probing over 64-byte
// entries; the table is not written while the kernel runs) and writes its key
// id, column words, valid bytes and spelling; a fallback record writes
// HSG_KEY_NONE and zeros, and its index goes to the fallback list at the
// tile's offset from the chained scan, so the list is in record order.
//
// Byte model per record of L bytes and C columns: read L + 8 (the bytes, one
// offset) and one 64-byte table entry per probe (one at load <= 1/2, mostly);
// written 4 (key) + 9 C (+ 4 with spellings), and 4 per fallback record;
// 8 B of tile state per 256 records each way and one ticket atomic per tile.
//
// k_ingest_patch scatters the host decoder's rows of the fallback records
// over theirs; k_ingest_table_put writes the key-table entries the host built
// at the slots the host chose.
#include "hsg_ingest.h"
#include "hsg_lookback.h"

namespace hsg {

namespace {

constexpr int T = kIngestTile;
using namespace lookback;

// the key's id (HSG_KEY_NONE: absent) and its first spelling's form
__device__ __forceinline__ uint32_t table_find(const jf::KeyEntry *table, uint64_t mask, uint8_t tag, uint8_t len,
                                               const uint64_t (&w)[6], uint8_t &form) {
  const uint64_t h = jf::key_hash(tag, len, w);
  uint64_t q = h & mask;
  for (uint64_t probes = 0; probes <= mask; ++probes) {
    const jf::KeyEntry *e = table + q;
    const uint32_t id1 = e->id1;
    if (!id1) return HSG_KEY_NONE;
    if (e->hash == h && e->tag == tag && e->len == len) {
      bool eq = true;
#pragma unroll
      for (int k = 0; k < 6; ++k) eq = eq && e->w[k] == w[k];
      if (eq) {
        form = e->form;
        return id1 - 1;
      }
    }
    q = (q + 1) & mask;
  }
  return HSG_KEY_NONE;
}

}  // namespace

template <int C>
__global__ __launch_bounds__(T) void k_json_decode(const IngestArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_buf[kIngestLds];
  __shared__ jf::Targets s_t;
  __shared__ TileLds<T / 64> s_lds;

  const int tid = threadIdx.x;
  for (uint32_t k = tid; k < sizeof(jf::Targets) / 4; k += T)
    reinterpret_cast<uint32_t *>(&s_t)[k] = reinterpret_cast<const uint32_t *>(a.tg)[k];
  const uint64_t n_tiles = (a.n + T - 1) / T;
  const uint64_t base0 = a.off[0];

  while (true) {
    // (the barrier inside also orders s_t and the last tile's s_buf reads)
    const uint64_t t = take_tile(s_lds, a.state);
    if (t >= n_tiles) return;
    const uint64_t r0 = t * T, r1 = r0 + T < a.n ? r0 + T : a.n;
    const uint64_t i = r0 + tid;
    const bool in = i < r1;
    const uint64_t b0 = a.off[r0] - base0, b1 = a.off[r1] - base0;
    const uint64_t lo = b0 & ~15ull, hi = (b1 + 15) & ~15ull;
    const bool staged = hi - lo <= kIngestLds;  // uniform
    if (staged) {
      for (uint64_t k = (uint64_t)tid * 16; k < hi - lo; k += (uint64_t)T * 16)
        *reinterpret_cast<uint4 *>(s_buf + k) = *reinterpret_cast<const uint4 *>(a.buf + lo + k);
    }
    __syncthreads();

    jf::Scan r;
    r.accept = 0;
    uint32_t key = HSG_KEY_NONE;
    if (in) {
      const uint64_t o0 = a.off[i] - base0, o1 = a.off[i + 1] - base0;
      if (o1 - o0 <= jf::kMaxRecord) {
        const uint8_t *p = staged ? s_buf + (o0 - lo) : a.buf + o0;
        jf::scan_record<C>(p, (uint32_t)(o1 - o0), s_t, r);
        if (r.accept) {
          if (s_t.keyless) {
            key = 0;
          } else {
            uint64_t w[6];
            const uint8_t len = jf::key_payload(p, r, w);
            uint8_t form = 0;
            key = table_find(a.table, a.table_mask, r.key_tag, len, w, form);
            // a number spelled unlike the key's first spelling: the host assigns the alternate
            if (key != HSG_KEY_NONE && a.spell && r.key_tag == 'n' && form != (r.key_iform ? 'i' : 'd'))
              key = HSG_KEY_NONE;
          }
        }
      }
    }
    const bool ok = key != HSG_KEY_NONE;
    const Rank k = rank_kept(s_lds, in && !ok);
    const uint64_t excl = publish_tile(s_lds, a.state + 2, t, n_tiles, k.count, a.sc, ERR_INGEST,
                                       &a.sc->scratch[kIngestWord], kIngestRan);
    if (excl == kNoSum) return;  // uniform
    if (in) {
      a.key_id[i] = key;
      if (a.spell) a.spell[i] = key;
#pragma unroll
      for (int c = 0; c < C; ++c)
        if (c < s_t.n_cols) {
          a.col[c][i] = ok ? (int64_t)r.word[c] : 0;
          a.valid[c][i] = ok ? r.valid[c] : (uint8_t)0;
        }
      if (!ok) a.list[excl + k.rank] = (uint32_t)i;
    }
    __syncthreads();  // s_buf and s_lds are reused by the next tile
  }
}

__global__ __launch_bounds__(256) void k_ingest_patch(const IngestPatch a) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.cnt) return;
  const uint64_t i = a.list[j];
  a.key_id[i] = a.h_key[j];
  if (a.spell) a.spell[i] = a.h_spell[j];
#pragma unroll
  for (int c = 0; c < kMaxCols; ++c)
    if (c < a.n_cols) {
      a.col[c][i] = a.h_col[c][j];
      a.valid[c][i] = a.h_valid[c][j];
    }
}

__global__ __launch_bounds__(256) void k_ingest_table_put(jf::KeyEntry *table, const uint64_t *slot,
                                                          const jf::KeyEntry *ents, uint64_t n) {
  // four lanes an entry, 16 bytes each
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t j = g >> 2;
  if (j >= n) return;
  const uint32_t part = (uint32_t)(g & 3);
  reinterpret_cast<uint4 *>(table + slot[j])[part] = reinterpret_cast<const uint4 *>(ents + j)[part];
}

void launch_json_decode(hipStream_t s, int n_cols, const IngestArgs &a) {
  if (!a.n) return;
  // a workgroup per tile up to a resident round; the workgroups take tiles until none is left
  const uint64_t tiles = (a.n + T - 1) / T;
  const dim3 grid((unsigned)(tiles < 2048 ? tiles : 2048));
  if (n_cols == 0) hipLaunchKernelGGL(k_json_decode<0>, grid, dim3(T), 0, s, a);
  else if (n_cols == 1) hipLaunchKernelGGL(k_json_decode<1>, grid, dim3(T), 0, s, a);
  else if (n_cols == 2) hipLaunchKernelGGL(k_json_decode<2>, grid, dim3(T), 0, s, a);
  else if (n_cols <= 4) hipLaunchKernelGGL(k_json_decode<4>, grid, dim3(T), 0, s, a);
  else hipLaunchKernelGGL(k_json_decode<8>, grid, dim3(T), 0, s, a);
}

void launch_ingest_patch(hipStream_t s, const IngestPatch &a) {
  if (!a.cnt) return;
  hipLaunchKernelGGL(k_ingest_patch, dim3((unsigned)((a.cnt + 255) / 256)), dim3(256), 0, s, a);
}

void launch_ingest_table_put(hipStream_t s, jf::KeyEntry *table, const uint64_t *slot, const jf::KeyEntry *ents,
                             uint64_t n) {
  if (!n) return;
  hipLaunchKernelGGL(k_ingest_table_put, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, s, table, slot, ents, n);
}

}  // namespace hsg
