// npr_scan.hip -- the prefix sums of npr_scan.h as the units use them: the kernels are compiled here, once per pair of types
#include "npr_scan.h"

namespace npr {

int64_t scan_tiles(int64_t n) { return n / SCAN_TILE + 1; }  // entries 0 .. n: the total has a place of its own

template int launch_scan_group<uint32_t, int64_t>(const uint32_t *, int64_t *, int64_t, void *);  // npr_seedmap.hip: hit_off; npr_snpcall.hip: tile_off
template int launch_scan_group<int64_t, int64_t>(const int64_t *, int64_t *, int64_t, void *);    // npr_seedmap.hip: chain_off; npr_seedchain.hip: n_ops
template int launch_scan_tiled<uint32_t, int32_t>(const uint32_t *, int32_t *, int64_t, int32_t *, void *);  // npr_bam.hip: the digit histograms, the run heads
template int launch_scan_tiled<int64_t, int64_t>(const int64_t *, int64_t *, int64_t, int64_t *, void *);  // npr_cigtext.hip: str_off

}  // namespace npr
