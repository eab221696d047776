// k_wall_regions_joint.hip -- BUILD-DEFINED EXTENSION: connected deviation regions of a window of the wall alignment's global
// station grid (gm_wall_alignment_regions), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_alignment_regions_np.py.  These are the
// joint instantiations of the two region kernels that read a cell of a map (gm_wall_regions.hpp): window row j is station
// station0 + (j - row0) of the piece that holds it, one element map (and its baseline's) per piece, the table of pieces in
// device memory (a window may meet every element).  The tiles kernel finds the piece of its first row by one binary search
// per block and walks forward as its rows advance; the reduce searches for the flagged cells alone.  Seams, flatten,
// select and labels work on the window-local scratch and are k_wall_regions.hip's, unchanged: a.first is the global index
// of window cell 0, so labels, peak cells and stations come out global.  A piece is checked before anything is read
// through it, and the host has checked every piece against its map: every map index is < n_stations_e n_sectors by
// construction, nothing is clamped.  No floating point anywhere.
#include "gm_wall_regions.hpp"

namespace gm {

__global__ __launch_bounds__(kCcThreads) void k_wall_region_tiles_joint(WallRegionArgs a) { wr_tiles<WrPieceCells>(a); }
__global__ __launch_bounds__(kCcThreads) void k_wall_region_reduce_joint(WallRegionArgs a) { wr_reduce<WrPieceCells>(a); }

void launch_wall_region_tiles_joint(const WallRegionArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_tiles_joint, dim3(a.tiles_s * a.tiles_k), dim3(kCcThreads), 0, s, a);
}
void launch_wall_region_reduce_joint(const WallRegionArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_region_reduce_joint, dim3(cc_blocks((uint64_t)a.n * a.nsec)), dim3(kCcThreads), 0, s, a);
}

}  // namespace gm
