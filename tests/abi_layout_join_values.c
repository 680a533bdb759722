/* Offsets and sizes of the valued join's structs (include/hstream_join.h), printed
 * as "type.member offset" / "type.sizeof size" for tests/test_join_values_host.py,
 * which compares them with the ctypes mirror in hstream_amd/abi.py. */
#include <stddef.h>
#include <stdio.h>
#include "hstream_join.h"
#define F(t, f) printf(#t "." #f " %zu\n", offsetof(t, f))
int main(void) {
  F(hsg_join_values, n_cols); F(hsg_join_values, col_types);
  F(hsg_join_cols, cols); F(hsg_join_cols, valid);
  F(hsg_join_joined, capacity); F(hsg_join_joined, mem); F(hsg_join_joined, key_col); F(hsg_join_joined, key_id);
  F(hsg_join_joined, ts); F(hsg_join_joined, cols); F(hsg_join_joined, valid); F(hsg_join_joined, this_handle);
  F(hsg_join_joined, other_handle); F(hsg_join_joined, join_key);
  printf("hsg_join_values.sizeof %zu\n", sizeof(hsg_join_values));
  printf("hsg_join_cols.sizeof %zu\n", sizeof(hsg_join_cols));
  printf("hsg_join_joined.sizeof %zu\n", sizeof(hsg_join_joined));
  printf("hsg_join_batch.sizeof %zu\n", sizeof(hsg_join_batch));
  printf("hsg_join_rows.sizeof %zu\n", sizeof(hsg_join_rows));
  printf("HSG_JOIN_MAX_COLS %d\n", HSG_JOIN_MAX_COLS);
  return 0;
}
