// The split predict kernels, double generation, round 3's two-phase step: one translation unit per slice of leaf_split.hpp's
// instantiations, so that they compile in parallel.
#include <hip/hip_runtime.h>

#include "leaf_split.hpp"

namespace gpso {
template int launch_leaf_tiles_bf16_v<double, false, 0>(hipStream_t, const KernParams&, const SplitLeafLaunch<double>&);
template int launch_leaf_tiles_bf16_v<double, false, 1>(hipStream_t, const KernParams&, const SplitLeafLaunch<double>&);
}  // namespace gpso
