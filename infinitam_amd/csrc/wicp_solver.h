// wicp_solver.h -- host side of the weighted ICP tracker: the undamped Gauss-Newton loop of ITMWeightedICPTracker::TrackCamera.
// Plain C++ (no HIP), shared by tracker.hip (weighted cost / gradient / Hessian evaluated on the GPU) and by the host-only hook
// itm_debug_wicp_track (tests/test_wicp_tracker.py).
//
// Behaviour of ITMWeightedICPTracker::TrackCamera / ComputeDelta / ApplyDelta / HasConverged (Engine/ITMWeightedICPTracker.cpp:102-191),
// own formulation: the level schedule of the ICP tracker (icp_track: coarse to fine down to noICPRunTillLevel, 2 (l + 1) iterations
// on level l, the same distance-threshold ramp); per iteration { evaluate at the current pose; stop the level when nothing is valid;
// solve H x = nabla for the active 3 or 6 parameters -- no damping, no accept / reject, H and nabla NOT divided by the valid count;
// apply x as ICP does (apply_first_order_step: first-order motion on the left of the inverse pose, projected onto SE(3)); stop the
// level when |x| / 6 < terminationThreshold }.  Poses and the solve in double (se3.h).
//
// The reference also leaves a level when f_new > f_old, but f_old is initialised to 1e10 and never assigned, and f is at most 1e5:
// that test never fires, and is not restated here.
//
// One deliberate divergence: where H is singular (e.g. every valid pixel has weight 0, so H = 0 while the valid count is positive)
// the reference's float Cholesky divides by a zero pivot and its pose becomes non-finite; here se3::solve_spd reports the singular
// system, no step is taken and the level ends.
#pragma once

#include <cmath>

#include "../../include/itm_hip.h"
#include "icp_solver.h"
#include "se3.h"

namespace itm {

// `evaluate(level, mode, inversePose16, distThresh, out)` returns the weighted sums at a pose (0 = ok)
template <class Evaluate>
inline int wicp_track(const itm_tracker_config* cfg, const float M_d_in[16], float M_d_out[16], Evaluate&& evaluate) {
  const int levels = cfg->noHierarchyLevels;
  se3::Rigid pose = se3::from_matrix(M_d_in);
  for (int level = levels - 1; level >= cfg->noICPRunTillLevel; --level) {
    const int mode = cfg->trackingRegime[level];
    if (mode == ITM_TRACKER_ITERATION_NONE) continue;
    const int maxIterations = 2 * (level + 1);
    float distThresh = cfg->distThresh;
    for (int l = levels - 1; l > level; --l) distThresh -= cfg->distThresh / (float)levels;
    const int n = (mode == ITM_TRACKER_ITERATION_BOTH) ? 6 : 3;
    for (int k = 0; k < maxIterations; ++k) {
      float invPose[16];
      se3::Rigid inv;
      if (!se3::invert(pose, inv)) inv = pose;
      se3::to_matrix(inv, invPose);
      itm_tracker_gh e;
      const int rc = evaluate(level, mode, invPose, distThresh, &e);
      if (rc) return rc;
      if (e.noValidPoints <= 0) break;
      // ComputeDelta: H x = nabla on the top-left n x n block (hessian[r + c * 6] is symmetric: row- and column-major alike)
      double H[36], g[6], x[6] = {0, 0, 0, 0, 0, 0};
      for (int i = 0; i < 36; ++i) H[i] = (double)e.hessian[i];
      for (int i = 0; i < 6; ++i) g[i] = (double)e.nabla[i];
      if (!se3::solve_spd(H, 6, n, g, x)) break;
      apply_first_order_step(pose, x, mode);
      double len = 0.0;
      for (int i = 0; i < 6; ++i) len += x[i] * x[i];
      if (std::sqrt(len) / 6.0 < (double)cfg->terminationThreshold) break;
    }
  }
  se3::to_matrix(pose, M_d_out);
  return 0;
}

}  // namespace itm
