// The fast-subset scanner (hstream_amd/csrc/hsg_json.h) under the host
// sanitizers: a stand-alone program, built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan
//       -I hstream_amd/csrc tools/json_fast_check.cpp -o json_fast_check
// It runs the scanner over every record of a corpus file (tests/jsongen.py
// write_corpus_file) and over every prefix of each record, each copied into a
// heap block of exactly its size, so one byte read at or past p + len is an
// AddressSanitizer report. It prints the counts; exit status 0 = clean.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hsg_json.h"

using namespace hsg;

namespace {

struct Reader {
  const std::vector<uint8_t> &b;
  size_t at = 0;
  bool ok = true;
  uint32_t u32() {
    uint32_t v = 0;
    if (at + 4 > b.size()) return ok = false, 0u;
    memcpy(&v, b.data() + at, 4);
    at += 4;
    return v;
  }
  const uint8_t *bytes(size_t n) {
    if (at + n > b.size()) return ok = false, nullptr;
    const uint8_t *p = b.data() + at;
    at += n;
    return p;
  }
};

bool scan_copy(const uint8_t *src, uint32_t len, const jf::Targets &t, jf::Scan &r) {
  uint8_t *blk = (uint8_t *)malloc(len);  // exactly len bytes: nothing to read beyond
  if (len && !blk) abort();
  if (len) memcpy(blk, src, len);
  jf::scan_record<jf::kMaxCols>(blk, len, t, r);
  free(blk);
  return r.accept != 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s corpus-file [max prefix records]\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) return perror(argv[1]), 2;
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) file.insert(file.end(), chunk, chunk + n);
  fclose(f);
  const uint64_t prefix_records = argc > 2 ? strtoull(argv[2], nullptr, 10) : ~0ull;

  Reader rd{file};
  if (rd.u32() != 0x4A534643u) return fprintf(stderr, "not a corpus file\n"), 2;
  jf::Targets t;
  memset(&t, 0, sizeof(t));
  t.keyless = (uint8_t)rd.u32();
  t.literal_forms = (uint8_t)rd.u32();
  const uint32_t nc = rd.u32();
  if (nc > (uint32_t)jf::kMaxCols) return fprintf(stderr, "too many columns\n"), 2;
  t.n_cols = (uint8_t)nc;
  for (uint32_t k = 0; k <= nc; ++k) {
    if (k) {
      if (rd.u32() == 1u) t.f64_mask |= (uint8_t)(1u << (k - 1));  // HSG_F64
      if (rd.u32()) t.num_mask |= (uint8_t)(1u << (k - 1));
    }
    const uint32_t ln = rd.u32();
    const uint8_t *nm = rd.bytes(ln);
    if (!rd.ok || ln > jf::kMaxName) return fprintf(stderr, "bad field name\n"), 2;
    memcpy(t.name[k], nm, ln);
    t.len[k] = (uint8_t)ln;
  }
  const uint32_t n = rd.u32();
  uint64_t accepted = 0, prefixes = 0, prefix_accepted = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t len = rd.u32();
    const uint8_t *p = rd.bytes(len);
    if (!rd.ok) return fprintf(stderr, "truncated corpus file\n"), 2;
    jf::Scan r;
    accepted += scan_copy(p, len, t, r);
    if (i < prefix_records)
      for (uint32_t l = 0; l < len; ++l) {
        ++prefixes;
        prefix_accepted += scan_copy(p, l, t, r);
      }
  }
  printf("records %u accepted %llu prefixes %llu prefix_accepted %llu\n", n, (unsigned long long)accepted,
         (unsigned long long)prefixes, (unsigned long long)prefix_accepted);
  return 0;
}
