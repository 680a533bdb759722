/* Offsets and sizes of the device decoder's structs (include/hstream_ingest.h),
 * printed as "type.member offset" / "type.sizeof size" for
 * tests/test_ingest_fast_host.py, which compares them with the ctypes mirror in
 * hstream_amd/abi.py. hsg_sink_spellings is declared in hstream_ingest.h, which
 * hstream_sink.h includes; both are included here as a caller of the sink would. */
#include <stddef.h>
#include <stdio.h>
#include "hstream_sink.h"
#include "hstream_ingest.h"
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  F(hsg_gpu_decode_stats, records); F(hsg_gpu_decode_stats, accepted); F(hsg_gpu_decode_stats, host_records);
  F(hsg_gpu_decode_stats, new_keys); F(hsg_gpu_decode_stats, table_slots); F(hsg_gpu_decode_stats, table_rebuilds);
  F(hsg_json_probe, accept); F(hsg_json_probe, key_tag); F(hsg_json_probe, key_neg); F(hsg_json_probe, key_e);
  F(hsg_json_probe, key_m); F(hsg_json_probe, key_off); F(hsg_json_probe, key_len); F(hsg_json_probe, key_int_form);
  F(hsg_json_probe, words); F(hsg_json_probe, valid);
  F(hsg_sink_spellings, spell); F(hsg_sink_spellings, n); F(hsg_sink_spellings, src_base); F(hsg_sink_spellings, mem);
  printf("hsg_gpu_decode_stats.sizeof %zu\n", sizeof(hsg_gpu_decode_stats));
  printf("hsg_json_probe.sizeof %zu\n", sizeof(hsg_json_probe));
  printf("hsg_sink_spellings.sizeof %zu\n", sizeof(hsg_sink_spellings));
  return 0;
}
