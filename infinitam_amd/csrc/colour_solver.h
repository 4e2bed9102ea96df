// colour_solver.h -- host side of the colour tracker: Levenberg-Marquardt over SE(3) on the photometric cost.  Plain C++ (no
// HIP); colour_tracker.hip evaluates the cost, gradient and Hessian on the GPU.
//
// Behaviour of ITMColorTracker::TrackCamera / minimizeLM / ApplyDelta (Engine/ITMColorTracker.cpp:25-47,70-234), own formulation:
//   * the pose is the rgb camera's world -> camera motion, calib_inv * pose_d on entry, calib * M (then coerced) on exit;
//   * per level, coarse to fine: trust-region LM with lambda starting at 0.01, the diagonal scaled by (1 + lambda) (an entry below
//     1e-15 in magnitude replaced by lambda * 1e-10), the step -d from (H + damping) d = g, accepted when the gain ratio rho is
//     above 0.25 (lambda / 2 above 0.75, lambda * 4 at or below 0.25); the level ends when max |d| < 5e-5, when an accepted step
//     lowers f by less than |f| * 1e-5, or after 100 steps;
//   * the step is the exponential of the 6-vector (translation, rotation) -- ROTATION fills the rotation part from the 3-parameter
//     solve, TRANSLATION the translation part from the first three of the full 6-parameter solve (the reference's quirk) --
//     applied on the left of the current pose;
//   * poses and the solve in double (se3.h).
// Every evaluation returns f together with the gradient and Hessian at the same pose (one pass over the points): the reference
// asks for them only once a step is accepted, which the loop then does without a second pass.
#pragma once

#include <cmath>
#include <cstring>

#include "../../include/itm_hip.h"
#include "se3.h"

namespace itm {

struct ColourPoint {          // an evaluated pose: the EvaluationPoint of the reference
  se3::Rigid pose;
  double f = 0.0;
  double g[6] = {0, 0, 0, 0, 0, 0};
  double H[36] = {};          // hessian[para + col * numPara]
};

constexpr int kColourMaxSteps = 100;
constexpr double kColourMinStep = 0.00005f;          // float constants of the reference, as float
constexpr double kColourMinDecrease = 0.00001f;

inline int colour_num_para(int mode) { return (mode == ITM_TRACKER_ITERATION_ROTATION) ? 3 : 6; }

// new = exp(delta as (translation, rotation)) * old
inline se3::Rigid colour_apply_delta(const se3::Rigid& old, const double* delta, int mode) {
  se3::Twist x = {{0, 0, 0}, {0, 0, 0}};
  for (int i = 0; i < 3; ++i) {
    if (mode == ITM_TRACKER_ITERATION_ROTATION) x.w[i] = (float)delta[i];
    else x.v[i] = (float)delta[i];
    if (mode == ITM_TRACKER_ITERATION_BOTH) x.w[i] = (float)delta[3 + i];
  }
  return se3::compose(se3::exp(x), old);
}

// `evaluate(level, mode, pose16, out)` fills out.f / g / H at the float matrix of out.pose (0 = ok).
template <class Evaluate>
inline int colour_minimize_level(int level, int mode, se3::Rigid& pose, Evaluate&& evaluate, int* evaluations) {
  const int n = colour_num_para(mode);
  ColourPoint x, x2;
  x.pose = pose;
  int rc = evaluate(level, mode, x);
  ++*evaluations;
  if (rc) return rc;
  if (!std::isfinite(x.f)) return ITM_OK;
  float lambda = 0.01f;
  for (int step = 0;; ++step) {
    double A[36], d[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n * n; ++i) A[i] = x.H[i];
    for (int i = 0; i < n; ++i) {
      double& a = A[i * (n + 1)];
      if (!(std::fabs(a) < 1e-15)) a *= 1.0 + (double)lambda;
      else a = (double)lambda * 1e-10;
    }
    se3::solve_spd(A, n, n, x.g, d);             // symmetric: the column-major layout reads the same as row-major
    double maxNorm = 0.0;
    for (int i = 0; i < n; ++i) maxNorm = std::fmax(maxNorm, std::fabs(d[i]));
    if (maxNorm < kColourMinStep) break;
    for (int i = 0; i < n; ++i) d[i] = -d[i];
    x2.pose = colour_apply_delta(x.pose, d, mode);
    rc = evaluate(level, mode, x2);
    ++*evaluations;
    if (rc) return rc;
    // gain ratio: actual / predicted reduction of the quadratic model
    double predicted = 0.0;
    for (int i = 0; i < n; ++i) {
      double Bd = 0.0;
      for (int j = 0; j < n; ++j) Bd += x.H[i + j * n] * d[j];
      predicted -= x.g[i] * d[i] + 0.5 * d[i] * Bd;
    }
    const double actual = x.f - x2.f;
    const double rho = actual / ((predicted < 0) ? std::fabs(predicted) : predicted);
    bool success = true;
    if (rho > 0.75) lambda = lambda / 2.0f;
    else if (rho <= 0.25) { success = false; lambda = lambda / 0.25f; }
    if (success) {
      const bool more = x2.f < x.f - std::fabs(x.f) * kColourMinDecrease;
      x = x2;
      if (!more) break;
    }
    if (step >= kColourMaxSteps - 1) break;
  }
  pose = x.pose;
  return ITM_OK;
}

// TrackCamera: M_d_in = pose_d, calib = trafo_rgb_to_depth.calib, calibInv = its calib_inv; writes the coerced pose_d.
template <class Evaluate>
inline int colour_track(const itm_tracker_config* cfg, const float M_d_in[16], const float calib[16], const float calibInv[16],
                        float M_d_out[16], Evaluate&& evaluate, int* evaluations) {
  *evaluations = 0;
  const se3::Rigid C = se3::from_matrix(calib), Ci = se3::from_matrix(calibInv);
  se3::Rigid pose = se3::compose(Ci, se3::from_matrix(M_d_in));
  for (int level = cfg->noHierarchyLevels - 1; level >= 0; --level) {
    const int rc = colour_minimize_level(level, cfg->trackingRegime[level], pose, evaluate, evaluations);
    if (rc) return rc;
  }
  se3::to_matrix(se3::exp(se3::log(se3::compose(C, pose))), M_d_out);
  return ITM_OK;
}

}  // namespace itm
