// Explicit instantiation of the channel-tiled spatial stage (spatial_wide.inc) for one (dtype, per-head) combination.
#include "spatial_wide.inc"

namespace sttm {
template hipError_t launch_spatial_wide_t<f16_t, true>(const SpatialArgs&, const BatchPtrs&, int, int, int, int, hipStream_t);
}  // namespace sttm
