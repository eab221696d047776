// k_wall_objects_joint.hip -- BUILD-DEFINED EXTENSION: a check's changed points as objects on the alignment's global station
// grid (gm_wall_alignment_check_objects, gm_wall_alignment_check_objects_rows), the device side.
//
// The rule is stated in include/gm_hip.h and DESIGN.md; the CPU twin is tests/wall_alignment_objects_np.py.  These are the
// joint instantiations of the three kernels that read a row: the decode (gm_wall_objects.hpp) checks the row's side
// against the by-value side table BEFORE the side picks anything, checks the cell against that side's own cell count, and
// turns (side, j) into the global station G = first[side] + j; from there on bin, reduce and rows are the map's code on a
// virtual map of `total` stations.  Tiles, seams, flatten, blocks and select never see a cell and are
// k_wall_objects.hip's, unchanged.  The bin also counts the rows of each side that are not rejected (counter words
// 9 .. 12).  Every store index is a row index < n_rows, an index < 2 NB or a slot < the component count by construction;
// nothing is clamped.  Integer arithmetic only after the two fixed-point conversions of a row.
#include "gm_wall_objects.hpp"

namespace gm {

__global__ __launch_bounds__(kCcThreads) void k_wall_object_bin_joint(WallObjectArgs a) { wo_bin<true>(a); }
__global__ __launch_bounds__(kCcThreads) void k_wall_object_reduce_joint(WallObjectArgs a) { wo_reduce<true>(a); }
__global__ __launch_bounds__(kCcThreads) void k_wall_object_rows_joint(WallObjectArgs a) { wo_rows<true>(a); }

void launch_wall_object_bin_joint(const WallObjectArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_object_bin_joint, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_object_reduce_joint(const WallObjectArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_object_reduce_joint, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
}
void launch_wall_object_rows_joint(const WallObjectArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_wall_object_rows_joint, dim3(cc_blocks(a.n_rows)), dim3(kCcThreads), 0, s, a);
}

}  // namespace gm
