// F_LAF_check (matching.cpp:192-249), shared by the two F verifiers (mods_loransac_f, mods_orsa_f): correspondence i of cur
// survives when its centre and the two frame points k_sigma along the local affine frame's axes, in both images, have a summed
// square-rooted epipolar error of at most `bound` (LAFCoef * err_threshold) under F (degensac's layout, as ransac_corresp.H).
// fds: FDs for errorType Sampson, FDsSym otherwise.  laf: n x 14 frames; bound <= 0 or laf == NULL: nothing is checked.
#pragma once
#include <cmath>
#include <vector>

namespace mods {

inline void f_laf_check(const double *laf, const double *F, double bound, void (*fds)(const double *, const double *, double *, int),
                        std::vector<int> &cur) {
  if (!(bound > 0) || !laf) return;
  std::vector<int> good;
  const double ks = 3.0;   // k_sigma, matching.cpp:171
  for (int i : cur) {
    const double *f = laf + (size_t)i * 14;
    double u[18], err[3];
    u[0] = f[0]; u[1] = f[1]; u[2] = 1.0;
    u[3] = f[7]; u[4] = f[8]; u[5] = 1.0;
    u[6] = u[0] + ks * f[3] * f[6]; u[7] = u[1] + ks * f[5] * f[6]; u[8] = 1.0;
    u[9] = u[3] + ks * f[10] * f[13]; u[10] = u[4] + ks * f[12] * f[13]; u[11] = 1.0;
    u[12] = u[0] + ks * f[2] * f[6]; u[13] = u[1] + ks * f[4] * f[6]; u[14] = 1.0;
    u[15] = u[3] + ks * f[9] * f[13]; u[16] = u[4] + ks * f[11] * f[13]; u[17] = 1.0;
    fds(u, F, err, 3);
    const double sumErr = std::sqrt(err[0]) + std::sqrt(err[1]) + std::sqrt(err[2]);
    if (!(sumErr > bound)) good.push_back(i);
  }
  cur.swap(good);
}

}  // namespace mods
