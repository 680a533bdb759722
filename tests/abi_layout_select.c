/* Offsets and sizes of the select op's structs (include/hstream_gpu.h), printed as
 * "type.member offset" / "type.sizeof size" for tests/test_select_host.py, which
 * compares them with the ctypes mirror in hstream_amd/abi.py. */
#include <stddef.h>
#include <stdio.h>
#include "hstream_gpu.h"
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  F(hsg_select_config, n_cols); F(hsg_select_config, flags); F(hsg_select_config, col_types);
  F(hsg_select_config, out_capacity);
  F(hsg_select_stats, where_dropped); F(hsg_select_stats, where_dropped_total); F(hsg_select_stats, expr_dropped);
  F(hsg_select_stats, expr_dropped_total); F(hsg_select_stats, having_dropped);
  F(hsg_select_stats, having_dropped_total); F(hsg_select_stats, emitted); F(hsg_select_stats, emitted_total);
  printf("hsg_select_config.sizeof %zu\n", sizeof(hsg_select_config));
  printf("hsg_select_stats.sizeof %zu\n", sizeof(hsg_select_stats));
  printf("hsg_stats.sizeof %zu\n", sizeof(hsg_stats));
  printf("hsg_op_config.sizeof %zu\n", sizeof(hsg_op_config));
  return 0;
}
