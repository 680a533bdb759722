// gfx950 kernels of the keyed view read (hsg_view_get): the rows of up to
// HSG_VIEW_MAX_KEYS keys out of an op's HBM state, without a scan of the whole
// table. What it replaces is the reference's only read of a view, SELECT ...
// FROM view WHERE key = x (SelectViewPlan, hstream/src/HStream/Server/
// Handler.hs:277-323: the store's rows of that key, Store.hs ksGet /
// findSessions).
//
// The layout does the work (hsg_tw.h, hsg_session.h):
//   time windows  every window of a key lives in the key's hash region of the
//                 table, or in the overflow rows: the scan covers the distinct
//                 regions of the requested keys and the overflow rows, a chunk
//                 of kEmitChunk slots per workgroup, and keeps the rows whose
//                 key word names a requested key (the sorted keys sit in LDS)
//   unwindowed    one tw_find per key
//   sessions      one find-only probe of the key table per key (ss_find); the
//                 key's list is contiguous and sorted by start
// Every read is count pass -> exclusive scan -> emit pass (as k_tw_emit_count /
// k_tw_emit_rows): no workgroup waits for another inside a launch, and a row's
// position depends only on the table, never on scheduling. The host reads the
// total between the two passes (the capacity rule of hsg_drain). Rows are
// rendered by the dump's out_value / out_form.
#include "hsg_dev.h"
#include "hsg_kernels.h"
#include "hsg_session.h"
#include "hsg_sort.h"
#include "hsg_tw.h"

namespace hsg {

// ---------------------------------------------------------------------------
// time windows: the requested keys' regions and the overflow rows
// ---------------------------------------------------------------------------
// slots [lo, hi) of chunk b
__device__ inline void view_chunk(const ViewScan &v, uint32_t b, uint64_t &lo, uint64_t &hi) {
  const uint32_t nrc = v.n_regions * v.cpr;
  uint64_t end;
  if (b < nrc) {
    const uint64_t base = v.region[b / v.cpr];
    lo = base + (uint64_t)(b % v.cpr) * kEmitChunk;
    end = base + v.rslots;
  } else {
    lo = v.ovf_base + (uint64_t)(b - nrc) * kEmitChunk;
    end = v.ovf_base + v.ovf_slots;
  }
  hi = lo + kEmitChunk < end ? lo + kEmitChunk : end;
  if (lo > hi) lo = hi;
}

// the request's keys into LDS (workgroup-wide; the caller synchronises)
__device__ inline void view_load_keys(uint32_t *sk, const uint32_t *__restrict__ keys, uint32_t nk) {
  for (uint32_t i = threadIdx.x; i < nk; i += blockDim.x) sk[i] = keys[i];
}
// sorted, distinct keys: binary search
__device__ inline bool view_has_key(const uint32_t *sk, uint32_t nk, uint32_t key) {
  uint32_t lo = 0, hi = nk;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (sk[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < nk && sk[lo] == key;
}
// slot s < hi holds a group of a requested key (a free slot's key word is
// kEmpty, whose key half is HSG_KEY_NONE: never in the list, checked anyway)
__device__ inline bool view_hit(const TwTable &t, uint64_t s, uint64_t hi, const uint32_t *sk, uint32_t nk) {
  if (s >= hi) return false;
  const uint64_t g = *t.key(s);
  return g != kEmpty && view_has_key(sk, nk, (uint32_t)(g >> 32));
}

__global__ __launch_bounds__(256) void k_view_tw_count(TwTable t, ViewScan v, const uint32_t *__restrict__ keys,
                                                       uint32_t nk, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t sk[HSG_VIEW_MAX_KEYS];
  __shared__ uint32_t sw[4];
  view_load_keys(sk, keys, nk);
  __syncthreads();
  uint64_t lo, hi;
  view_chunk(v, blockIdx.x, lo, hi);
  uint32_t h = 0;  // the wave's hits (uniform)
  for (uint64_t blk = lo; blk < hi; blk += 256)
    h += (uint32_t)__popcll(__ballot(view_hit(t, blk + threadIdx.x, hi, sk, nk)));
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = h;
  __syncthreads();
  if (threadIdx.x == 0) cnt[blockIdx.x] = sw[0] + sw[1] + sw[2] + sw[3];
}

__global__ __launch_bounds__(256) void k_view_tw_rows(TwTable t, ViewScan v, const uint32_t *__restrict__ keys,
                                                      uint32_t nk, Program prog, TwParams p,
                                                      const uint64_t *__restrict__ off, OutCols out, uint64_t out_cap,
                                                      DevScalars *sc) {
  __shared__ uint32_t sk[HSG_VIEW_MAX_KEYS];
  __shared__ uint32_t swave[4];
  view_load_keys(sk, keys, nk);
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t k_epoch = sc->k_epoch;
  uint64_t lo, hi;
  view_chunk(v, blockIdx.x, lo, hi);
  uint64_t run = off[blockIdx.x];
  for (uint64_t blk = lo; blk < hi; blk += 256) {
    const uint64_t s = blk + threadIdx.x;
    const bool hit = view_hit(t, s, hi, sk, nk);
    const uint64_t mask = __ballot(hit);
    if (lane == 0) swave[w] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint64_t o = run + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) o += swave[k];
    run += swave[0] + swave[1] + swave[2] + swave[3];
    __syncthreads();
    if (!hit || o >= out_cap) continue;
    const uint64_t g = *t.key(s);
    const int64_t *row = t.aggs(s);
    const int64_t k = k_epoch + (int64_t)(g & 0xFFFFFFFFull);
    const int64_t ws = (int64_t)((uint64_t)k * (uint64_t)p.adv);
    out.key[o] = (uint32_t)(g >> 32);
    out.ws[o] = ws;
    out.we[o] = (int64_t)((uint64_t)ws + (uint64_t)p.size);
    out.src[o] = -1;
    for (int j = 0; j < prog.n_out; ++j) out.agg[j][o] = out_value(prog, j, row);
    if (out.form) out.form[o] = out_form(prog, row);
  }
}

void launch_view_tw_count(hipStream_t s, const TwTable &t, const ViewScan &v, const uint32_t *keys, uint32_t nk,
                          const EmitScratch &es, uint64_t *total) {
  const uint64_t nb = v.chunks();
  hipLaunchKernelGGL(k_view_tw_count, dim3((unsigned)nb), dim3(256), 0, s, t, v, keys, nk, es.cnt);
  scan_excl_u32(s, es.cnt, es.off, nb, es.partial, total);
}

void launch_view_tw_rows(hipStream_t s, const TwTable &t, const ViewScan &v, const uint32_t *keys, uint32_t nk,
                         const Program &prog, const TwParams &p, const EmitScratch &es, OutCols out, uint64_t out_cap,
                         DevScalars *sc) {
  hipLaunchKernelGGL(k_view_tw_rows, dim3((unsigned)v.chunks()), dim3(256), 0, s, t, v, keys, nk, prog, p, es.off, out,
                     out_cap, sc);
}

// ---------------------------------------------------------------------------
// unwindowed ops and sessions: a lookup per key
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_view_kv_find(TwTable t, const uint32_t *__restrict__ keys, uint32_t nk,
                                                      int64_t *__restrict__ slot, uint32_t *__restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nk) return;
  const int64_t s = tw_find(t, (uint64_t)keys[i] << 32);  // the one implicit window: k = 0, epoch 0
  slot[i] = s;
  cnt[i] = s >= 0 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_view_ss_find(SessTable t, const uint32_t *__restrict__ keys, uint32_t nk,
                                                      int64_t *__restrict__ slot, uint32_t *__restrict__ cnt) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nk) return;
  const int64_t s = ss_find(t, keys[i]);
  slot[i] = s;
  cnt[i] = s >= 0 ? t.kt[s].len : 0u;
}

// off[i] = cnt[0] + ... + cnt[i - 1] for i <= nk <= HSG_VIEW_MAX_KEYS: one workgroup
__global__ __launch_bounds__(HSG_VIEW_MAX_KEYS) void k_view_scan(const uint32_t *__restrict__ cnt, uint32_t nk,
                                                                 uint64_t *__restrict__ off) {
  __shared__ uint64_t swave[HSG_VIEW_MAX_KEYS / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const uint64_t c = threadIdx.x < nk ? cnt[threadIdx.x] : 0;
  const uint64_t incl = wave_incl_sum(c);
  if (lane == 63) swave[w] = incl;
  __syncthreads();
  uint64_t before = 0;
  for (int k = 0; k < w; ++k) before += swave[k];
  if (threadIdx.x < nk) off[threadIdx.x] = before + incl - c;
  if (threadIdx.x + 1 == nk) off[nk] = before + incl;
}

__global__ __launch_bounds__(256) void k_view_kv_rows(TwTable t, Program prog, const uint32_t *__restrict__ keys,
                                                      uint32_t nk, const int64_t *__restrict__ slot,
                                                      const uint64_t *__restrict__ off, OutCols out,
                                                      uint64_t out_cap) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= nk) return;
  const int64_t s = slot[i];
  const uint64_t o = off[i];
  if (s < 0 || o >= out_cap) return;
  const int64_t *row = t.aggs((uint64_t)s);
  out.key[o] = keys[i];
  out.ws[o] = 0;
  out.we[o] = 0;
  out.src[o] = -1;
  for (int j = 0; j < prog.n_out; ++j) out.agg[j][o] = out_value(prog, j, row);
  if (out.form) out.form[o] = out_form(prog, row);
}

// a key's list: kViewLanes lanes take its sessions in turn (a list is tens of
// rows of 3 + slots words), so the rows of a list leave in start order
constexpr int kViewLanes = 16;
__global__ __launch_bounds__(256) void k_view_ss_rows(SessTable t, Program prog, const uint32_t *__restrict__ keys,
                                                      uint32_t nk, const int64_t *__restrict__ slot,
                                                      const uint64_t *__restrict__ off, OutCols out,
                                                      uint64_t out_cap) {
  const uint32_t i = (blockIdx.x * 256u + threadIdx.x) / kViewLanes;
  const uint32_t lane = threadIdx.x & (kViewLanes - 1);
  if (i >= nk) return;
  const int64_t s = slot[i];
  if (s < 0) return;
  const uint64_t o0 = off[i], len = off[i + 1] - o0, first = t.kt[s].off;
  for (uint64_t k = lane; k < len; k += kViewLanes) {
    const uint64_t o = o0 + k;
    if (o >= out_cap) return;
    const uint64_t *row = ss_row(t, first + k);
    out.key[o] = keys[i];
    out.ws[o] = (int64_t)row[0];
    out.we[o] = (int64_t)row[1];
    out.src[o] = -1;
    for (int j = 0; j < prog.n_out; ++j) out.agg[j][o] = out_value(prog, j, (const int64_t *)row + 3);
    if (out.form) out.form[o] = out_form(prog, (const int64_t *)row + 3);
  }
}

void launch_view_kv_find(hipStream_t s, const TwTable &t, const uint32_t *keys, uint32_t nk, int64_t *slot,
                         uint32_t *cnt) {
  hipLaunchKernelGGL(k_view_kv_find, dim3((nk + 255) / 256), dim3(256), 0, s, t, keys, nk, slot, cnt);
}
void launch_view_ss_find(hipStream_t s, const SessTable &t, const uint32_t *keys, uint32_t nk, int64_t *slot,
                         uint32_t *cnt) {
  hipLaunchKernelGGL(k_view_ss_find, dim3((nk + 255) / 256), dim3(256), 0, s, t, keys, nk, slot, cnt);
}
void launch_view_scan(hipStream_t s, const uint32_t *cnt, uint32_t nk, uint64_t *off) {
  hipLaunchKernelGGL(k_view_scan, dim3(1), dim3(HSG_VIEW_MAX_KEYS), 0, s, cnt, nk, off);
}
void launch_view_kv_rows(hipStream_t s, const TwTable &t, const Program &prog, const uint32_t *keys, uint32_t nk,
                         const int64_t *slot, const uint64_t *off, OutCols out, uint64_t out_cap) {
  hipLaunchKernelGGL(k_view_kv_rows, dim3((nk + 255) / 256), dim3(256), 0, s, t, prog, keys, nk, slot, off, out,
                     out_cap);
}
void launch_view_ss_rows(hipStream_t s, const SessTable &t, const Program &prog, const uint32_t *keys, uint32_t nk,
                         const int64_t *slot, const uint64_t *off, OutCols out, uint64_t out_cap) {
  hipLaunchKernelGGL(k_view_ss_rows, dim3((nk * kViewLanes + 255) / 256), dim3(256), 0, s, t, prog, keys, nk, slot, off,
                     out, out_cap);
}

}  // namespace hsg
