// SDF features on canonical points (ra_k4_canon.hpp) for bfloat16 operands.
#include "ra_k4_canon.hpp"
void launch_canonical_features_bf16(const GeoNet& net, const void* fwd_arena, const float* barena, const float* cpts, int n, float* feat, hipStream_t stream) {
    launch_canon_feat<bf16>(net, fwd_arena, barena, cpts, n, feat, stream);
}
