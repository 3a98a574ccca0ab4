// H_LAF_check (matching.cpp:250-308), shared by the two H verifiers (mods_loransac_h, mods_orsa_h); defined in capi.hip.
#pragma once
#include <vector>

namespace mods {
namespace rs { struct SimdOps; }

// correspondence i of cur survives when the symmetric transfer errors (HDsSymMax) of its centre and of the two frame points
// k_sigma along the local affine frame's axes sum to at most bound^2.  H21: the model from image 2 to image 1, row-major; laf:
// n x 14 frames; bound <= 0 or laf == NULL: nothing is checked.  ops: the host SIMD table, nullptr = the scalar statement.
void h_laf_check(const double *laf, const double *H21, double bound, const rs::SimdOps *ops, std::vector<int> &cur);
// the 3 x 3 inverse as the homography branch takes it (closed form in double; all zero and false on a zero determinant)
bool invert3x3(const double *S, double *t);

}  // namespace mods
