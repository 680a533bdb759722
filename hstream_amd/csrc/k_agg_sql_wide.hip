// The SQL lean kernels' variants for wide records and large programs
// (hsg_sql.h k_agg_sql_wide; the design is at the head of k_agg_sql.hip):
// packed records of 3 - 8 columns (5 - 10 words), slot programs of up to
// kMaxSlots = 24 slots. An instantiation unit of its own, as
// k_agg_s{2,4,6,8}.hip, so that it compiles beside k_agg_sql.hip.
//
// Variants (slot class: LDS entries, threads):
//   <= 12 slots   1024 entries, 1024 threads   (8 + 12 x 8 B per entry: 108 KiB)
//   <= 16 slots   1024 entries, 1024 threads   (140 KiB)
//   <= 24 slots    512 entries,  512 threads   (104 KiB; 1024 entries would
//                                               need 204 KiB of the 160)
// each for records of exactly 5 and 6 words (3 and 4 columns) and for any
// width (the column count read at run time, columns past it never loaded).
// Programs of 17 - 24 slots over one or two columns take the any-width
// variant of their class. sql_lds_entries (k_agg_sql.hip) returns the entries.
#include "hsg_sql.h"

namespace hsg {

template <int MS, int E, int NT>
static void sql_wide_launch(hipStream_t s, dim3 g, const Program &prog, const PartParams &pp, const TwTable &t,
                            const PartBuffers &pb, DevScalars *sc) {
  constexpr int RB = 4;  // records per thread per block
  const int W = pp.words - 1;
  if (W == 5)
    hipLaunchKernelGGL((k_agg_sql_wide<MS, E, NT, 5, RB>), g, dim3(NT), 0, s, prog, pp, t, pb, sc);
  else if (W == 6)
    hipLaunchKernelGGL((k_agg_sql_wide<MS, E, NT, 6, RB>), g, dim3(NT), 0, s, prog, pp, t, pb, sc);
  else
    hipLaunchKernelGGL((k_agg_sql_wide<MS, E, NT, 0, RB>), g, dim3(NT), 0, s, prog, pp, t, pb, sc);
}

void launch_sql_wide_agg(hipStream_t s, dim3 g, const Program &prog, const PartParams &pp, const TwTable &t,
                         const PartBuffers &pb, DevScalars *sc) {
  if (prog.n_slots <= 12) sql_wide_launch<12, 1024, 512>(s, g, prog, pp, t, pb, sc);
  else if (prog.n_slots <= 16) sql_wide_launch<16, 1024, 512>(s, g, prog, pp, t, pb, sc);
  else sql_wide_launch<24, 512, 512>(s, g, prog, pp, t, pb, sc);
}

void launch_sql_apply24(hipStream_t s, dim3 g, const Program &prog, const TwParams &p, const PartParams &pp,
                        const TwTable &t, const PartBuffers &pb, const OutCols &out, uint64_t out_base,
                        uint64_t out_cap, DevScalars *sc) {
  hipLaunchKernelGGL((k_sql_apply<24>), g, dim3(256), 0, s, prog, p, pp, t, pb, out, out_base, out_cap, sc);
}

}  // namespace hsg
