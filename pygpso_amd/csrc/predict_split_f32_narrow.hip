// The split predict kernels, the NARROW tile (4 waves x 1 column tile: 64 leaves per workgroup) of the default family -- float
// generation, fp16 split, fused step, fp16 contraction -- for all four kernel families: the survivors' launch of a screened
// best-UCB call (GPSO_OPT_SURVIVOR_TILE).  A translation unit of its own, so that the slices keep compiling in parallel.
#include <hip/hip_runtime.h>

#include "leaf_split.hpp"

namespace gpso {
int launch_leaf_tiles_narrow(hipStream_t st, const KernParams& kp, const SplitLeafLaunch<float>& a) {
  if (!leaf_narrow_applies(a, true)) {
    note_launch_error("launch_leaf_tiles_narrow: not a launch of the default family (fp16 split, fp16 contraction, fused step)");
    return 1;
  }
  const bool low = kp.kernel == 0 || kp.kernel == 1;
  return low ? launch_leaf_tiles_narrow_v<0>(st, kp, a) : launch_leaf_tiles_narrow_v<1>(st, kp, a);
}
}  // namespace gpso
