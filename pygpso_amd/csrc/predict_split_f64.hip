// The split predict kernels, double generation, the fused step: one translation unit per slice of leaf_split.hpp's
// instantiations, so that they compile in parallel.
#include <hip/hip_runtime.h>

#include "leaf_split.hpp"

namespace gpso {
template int launch_leaf_tiles_bf16_v<double, true, 0>(hipStream_t, const KernParams&, const SplitLeafLaunch<double>&);
template int launch_leaf_tiles_bf16_v<double, true, 1>(hipStream_t, const KernParams&, const SplitLeafLaunch<double>&);
}  // namespace gpso
