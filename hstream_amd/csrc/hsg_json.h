// The fast subset of the JSON ingest (include/hstream_ingest.h "GPU ingest"):
// one scanner over a record's bytes, compiled for the device (k_ingest.hip)
// and for the host (gpu_ingest.cpp's probe, tools/json_fast_check.cpp), and
// the device key table's entry and hash.
//
// The scanner's verdict is binary: it accepts a record only when it can prove
// what the host decoder (ingest.cpp decode_one) answers for it, and everything
// else -- malformed text, escapes, bytes outside 0x20-0x7E in a string, nested
// values, long numbers, values a column cannot hold -- is a fallback record
// that the host decoder sees whole. It assigns no reject status.
//
//   record  = ws '{' ws (member (ws ',' ws member)*)? ws '}' ws
//   member  = string ws ':' ws value
//   string  = '"' [0x20-0x7E except '"' '\']* '"'
//   value   = number | string | true | false | null
//
// A number of a decoded field (the key field or a configured column) is
// m * 10^se: m all integer and fraction digits read as one integer (at most
// kMaxDigits digits, so it fits a uint64_t), se the literal exponent (at most
// kMaxExpDigits digits) minus the count of fraction digits.
//   HSG_F64   m <= 2^53 and |se| <= 22: (double)m * 10^se or (double)m / 10^-se
//             is one IEEE operation on two exact doubles, so it is the
//             correctly rounded value strtod gives
//   HSG_I64   the value is integral and inside int64
//
// No recursion, no read at or beyond p + len, and no runtime-indexed
// per-thread array: the column state is unrolled over kMaxCols columns (the
// way hsg_pred.h keeps its stack in registers), the names live in memory the
// caller owns (kernel LDS, a host struct).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HSG_JHD __host__ __device__ inline
#else
#define HSG_JHD inline
#endif

#ifndef HSG_GPU_DEC_MAX_RECORD
#define HSG_GPU_DEC_MAX_RECORD 4096u
#define HSG_GPU_DEC_MAX_KEY 48u
#define HSG_GPU_DEC_MAX_COLS 8
#define HSG_GPU_DEC_MAX_NAME 64u
#endif

namespace hsg {
namespace jf {

constexpr int kMaxCols = HSG_GPU_DEC_MAX_COLS;
constexpr uint32_t kMaxName = HSG_GPU_DEC_MAX_NAME;
constexpr uint32_t kMaxKey = HSG_GPU_DEC_MAX_KEY;
constexpr uint32_t kMaxRecord = HSG_GPU_DEC_MAX_RECORD;
constexpr uint32_t kMaxDigits = 19, kMaxExpDigits = 3;

// The fields a decoder reads: name 0 is the key field, names 1 .. n_cols the
// columns. In HBM for the kernel, which copies it to LDS.
struct Targets {
  uint8_t name[kMaxCols + 1][kMaxName];
  uint8_t len[kMaxCols + 1];
  uint8_t keyless, literal_forms, n_cols;
  uint8_t f64_mask;  // bit c: column c is HSG_F64 (else HSG_I64)
  uint8_t num_mask;  // bit c: column c must hold a Number (else presence only)
  uint8_t pad[2];
};
static_assert(sizeof(Targets) == 592, "Targets layout");

// What the scanner found. The key's class: tag 'n' (neg, m without trailing
// zeros, e; zero is m = 0, e = 0, neg = 0; iform: its literal prints as an
// integer, se >= 0), 's' (the span [off, off + len) of the record), 'z' null,
// 't', 'f'; 0: no key member.
struct Scan {
  uint32_t accept;
  uint8_t key_tag, key_neg, key_iform, pad;
  int32_t key_e;
  uint64_t key_m;
  uint32_t key_off, key_len;
  uint64_t word[kMaxCols];
  uint8_t valid[kMaxCols];
};

struct Val {
  uint8_t kind;   // 0: not a value of the subset; 'n' 's' 't' 'f' 'z'
  uint8_t neg;
  uint8_t numok;  // the digit and exponent rule holds
  int32_t se;
  uint64_t m;
  uint32_t s_off, s_len;
};

HSG_JHD bool is_ws(uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r'; }
HSG_JHD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

HSG_JHD uint32_t skip_ws(const uint8_t *p, uint32_t len, uint32_t i) {
  while (i < len && is_ws(p[i])) ++i;
  return i;
}

// A subset string at p[i] == '"': its span; returns the index after the
// closing quote, or 0 (never a valid answer) when it is not one.
HSG_JHD uint32_t scan_string(const uint8_t *p, uint32_t len, uint32_t i, uint32_t &s_off, uint32_t &s_len) {
  ++i;
  s_off = i;
  while (i < len) {
    const uint8_t c = p[i];
    if (c == '"') {
      s_len = i - s_off;
      return i + 1;
    }
    if (c < 0x20 || c > 0x7E || c == '\\') return 0;
    ++i;
  }
  return 0;
}

// A value at p[i] (i < len): returns the index after it, v.kind = 0 when the
// text there is no value of the subset.
HSG_JHD uint32_t scan_value(const uint8_t *p, uint32_t len, uint32_t i, Val &v) {
  v.kind = 0;
  v.neg = 0;
  v.numok = 0;
  v.se = 0;
  v.m = 0;
  v.s_off = v.s_len = 0;
  const uint8_t c = p[i];
  if (c == '"') {
    const uint32_t j = scan_string(p, len, i, v.s_off, v.s_len);
    if (j) v.kind = 's';
    return j;
  }
  if (c == 't' || c == 'n') {
    if (len - i < 4) return 0;
    const bool ok = c == 't' ? (p[i + 1] == 'r' && p[i + 2] == 'u' && p[i + 3] == 'e')
                             : (p[i + 1] == 'u' && p[i + 2] == 'l' && p[i + 3] == 'l');
    if (!ok) return 0;
    v.kind = c == 't' ? 't' : 'z';
    return i + 4;
  }
  if (c == 'f') {
    if (len - i < 5) return 0;
    if (!(p[i + 1] == 'a' && p[i + 2] == 'l' && p[i + 3] == 's' && p[i + 4] == 'e')) return 0;
    v.kind = 'f';
    return i + 5;
  }
  // number: '-'? ('0' | [1-9][0-9]*) ('.' [0-9]+)? ([eE] [+-]? [0-9]+)?
  if (c == '-') {
    v.neg = 1;
    ++i;
  }
  if (i >= len || !is_digit(p[i])) return 0;
  uint32_t ndig = 0, nfrac = 0;
  uint64_t m = 0;
  if (p[i] == '0') {
    ++i;
    ndig = 1;
  } else {
    while (i < len && is_digit(p[i])) {
      if (++ndig <= kMaxDigits) m = m * 10 + (uint64_t)(p[i] - '0');
      ++i;
    }
  }
  if (i < len && p[i] == '.') {
    ++i;
    while (i < len && is_digit(p[i])) {
      if (++ndig <= kMaxDigits) m = m * 10 + (uint64_t)(p[i] - '0');
      ++nfrac;
      ++i;
    }
    if (!nfrac) return 0;
  }
  int32_t ex = 0;
  uint32_t nexp = 0;
  if (i < len && (p[i] == 'e' || p[i] == 'E')) {
    ++i;
    bool eneg = false;
    if (i < len && (p[i] == '+' || p[i] == '-')) eneg = p[i++] == '-';
    while (i < len && is_digit(p[i])) {
      if (++nexp <= kMaxExpDigits) ex = ex * 10 + (int32_t)(p[i] - '0');
      ++i;
    }
    if (!nexp) return 0;
    if (eneg) ex = -ex;
  }
  v.kind = 'n';
  v.numok = ndig <= kMaxDigits && nexp <= kMaxExpDigits;
  v.m = m;
  v.se = ex - (int32_t)(nfrac > 64u ? 64u : nfrac);  // (nfrac <= 19 whenever numok)
  return i;
}

HSG_JHD bool name_is(const uint8_t *p, uint32_t n_off, uint32_t n_len, const Targets &t, int k) {
  if (n_len != t.len[k]) return false;
  for (uint32_t j = 0; j < n_len; ++j)
    if (p[n_off + j] != t.name[k][j]) return false;
  return true;
}

// 10^k, k <= 19
HSG_JHD uint64_t pow10_u64(int k) {
  uint64_t r = 1;
  for (int j = 0; j < k; ++j) r *= 10;
  return r;
}
// 10^k as a double, k <= 22: every product is exact
HSG_JHD double pow10_f64(int k) {
  double r = 1.0;
  for (int j = 0; j < k; ++j) r *= 10.0;
  return r;
}

// A number into an HSG_F64 column: false = outside the rule.
HSG_JHD bool num_f64(const Val &v, uint64_t &word) {
  if (v.m > (1ull << 53) || v.se < -22 || v.se > 22) return false;
  double d = (double)v.m;
  d = v.se >= 0 ? d * pow10_f64(v.se) : d / pow10_f64(-v.se);
  if (v.neg) d = -d;
  word = __builtin_bit_cast(uint64_t, d);
  return true;
}

// A number into an HSG_I64 column: false = not integral or outside int64.
HSG_JHD bool num_i64(const Val &v, uint64_t &word) {
  const uint64_t lim = v.neg ? (1ull << 63) : (1ull << 63) - 1;
  uint64_t q = v.m;
  if (q == 0) {
    word = 0;
    return true;
  }
  if (v.se >= 0) {
    if (v.se > 19) return false;
    for (int j = 0; j < v.se; ++j) {
      if (q > lim / 10) return false;
      q *= 10;
    }
  } else {
    if (v.se < -19) return false;  // 10^-se > m
    const uint64_t d = pow10_u64(-v.se);
    if (q % d) return false;
    q /= d;
  }
  if (q > lim) return false;
  word = v.neg ? (uint64_t)0 - q : q;
  return true;
}

// The whole record. Every index read is below len. C: the columns matched
// (t.n_cols <= C), which bounds the unrolled column state.
template <int C = kMaxCols>
HSG_JHD void scan_record(const uint8_t *p, uint32_t len, const Targets &t, Scan &r) {
  r.accept = 0;
  r.key_tag = r.key_neg = r.key_iform = r.pad = 0;
  r.key_e = 0;
  r.key_m = 0;
  r.key_off = r.key_len = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int c = 0; c < kMaxCols; ++c) {
    r.word[c] = 0;
    r.valid[c] = 0;
  }
  if (len > kMaxRecord) return;
  uint32_t bad = 0;  // bit c: column c's last occurrence is outside its rule; bit 8: the key's
  uint32_t i = skip_ws(p, len, 0);
  if (i >= len || p[i] != '{') return;
  i = skip_ws(p, len, i + 1);
  if (i >= len) return;
  if (p[i] == '}') {
    ++i;
  } else {
    for (;;) {
      i = skip_ws(p, len, i);
      if (i >= len || p[i] != '"') return;
      uint32_t n_off, n_len;
      i = scan_string(p, len, i, n_off, n_len);
      if (!i) return;
      i = skip_ws(p, len, i);
      if (i >= len || p[i] != ':') return;
      i = skip_ws(p, len, i + 1);
      if (i >= len) return;
      Val v;
      i = scan_value(p, len, i, v);
      if (!i || !v.kind) return;
      if (n_len <= kMaxName) {
        const bool long_num = v.kind == 'n' && !v.numok;
        if (!t.keyless && name_is(p, n_off, n_len, t, 0)) {
          // the last occurrence wins
          r.key_tag = v.kind;
          r.key_off = v.s_off;
          r.key_len = v.s_len;
          r.key_neg = 0;
          r.key_m = 0;
          r.key_e = 0;
          r.key_iform = 0;
          bad &= ~256u;
          if (long_num || (v.kind == 's' && v.s_len > kMaxKey)) bad |= 256u;
          if (v.kind == 'n' && v.numok) {
            uint64_t m = v.m;
            int32_t e = v.se;
            while (m && m % 10 == 0) {
              m /= 10;
              ++e;
            }
            r.key_m = m;
            r.key_e = m ? e : 0;
            r.key_neg = (uint8_t)(v.neg && m);
            r.key_iform = (uint8_t)(v.se >= 0);
          }
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int c = 0; c < C; ++c) {
          if (c >= t.n_cols || !name_is(p, n_off, n_len, t, c + 1)) continue;
          uint64_t w = 0;
          uint8_t vb = 1;
          bool ok = !long_num;
          if (ok && ((t.num_mask >> c) & 1u)) {
            ok = v.kind == 'n' && (((t.f64_mask >> c) & 1u) ? num_f64(v, w) : num_i64(v, w));
            vb = (uint8_t)(1u | ((t.literal_forms && v.se < 0) ? 2u : 0u));
          }
          r.word[c] = ok ? w : 0;
          r.valid[c] = ok ? vb : (uint8_t)0;
          bad = ok ? (bad & ~(1u << c)) : (bad | (1u << c));
        }
      }
      i = skip_ws(p, len, i);
      if (i >= len) return;
      if (p[i] == '}') {
        ++i;
        break;
      }
      if (p[i] != ',') return;
      ++i;
    }
  }
  i = skip_ws(p, len, i);
  if (i != len) return;
  if (!t.keyless && !r.key_tag) return;  // the key field is absent
  if (bad) return;
  r.accept = 1;
}

// ---- device key table --------------------------------------------------------
// Open addressing over (tag, payload), linear probing, load at most 1/2. A
// number's payload is m (8 bytes), e (4 bytes), neg (1 byte); a string's its
// bytes; null / true / false have none.
struct KeyEntry {
  uint32_t id1;     // key id + 1; 0 = empty slot
  uint8_t tag, len, form, pad;  // form: 'i' / 'd' of a number's first spelling, else 0
  uint64_t hash;
  uint64_t w[6];    // payload, zero-padded
};
static_assert(sizeof(KeyEntry) == 64, "KeyEntry layout");

HSG_JHD uint64_t key_hash(uint8_t tag, uint8_t len, const uint64_t (&w)[6]) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ (((uint64_t)tag << 8 | len) * 0xff51afd7ed558ccdull);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 6; ++k) {
    h = (h ^ w[k]) * 0xbf58476d1ce4e5b9ull;
    h ^= h >> 31;
  }
  h *= 0x94d049bb133111ebull;
  h ^= h >> 29;
  return h;
}

// The payload of a scanned key. A number's is 13 bytes, a string's key_len.
HSG_JHD uint8_t key_payload(const uint8_t *p, const Scan &r, uint64_t (&w)[6]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int k = 0; k < 6; ++k) w[k] = 0;
  if (r.key_tag == 'n') {
    w[0] = r.key_m;
    w[1] = (uint64_t)(uint32_t)r.key_e | ((uint64_t)r.key_neg << 32);
    return 13;
  }
  if (r.key_tag == 's') {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < kMaxKey; ++j)
      if (j < r.key_len) w[j >> 3] |= (uint64_t)p[r.key_off + j] << (8 * (j & 7));
    return (uint8_t)r.key_len;
  }
  return 0;
}

}  // namespace jf
}  // namespace hsg
