// ren_solver.h -- host side of the Ren SDF tracker: the Levenberg-Marquardt loop of ITMRenTracker::TrackCamera over the pose
// parameters (translation, modified Rodrigues rotation).  Plain C++ (no HIP); ren_tracker.hip evaluates the energy, gradient and
// Hessian on the GPU.
//
// Behaviour of ITMRenTracker::TrackCamera / ComputeSingleStep / GetMFromParam / GetRotationMatrixFromMRP (Engine/ITMRenTracker.cpp),
// own formulation:
//   * level 0 only (the reference builds a coarser level it never reads and ignores the tracking regime);
//   * lambda starts at 1000; at most 100 outer steps, each at the current inverse pose invM;
//   * a step is -d from (H + damping) d = g, the diagonal scaled by (1 + lambda) (an entry below 1e-15 in magnitude replaced by
//     lambda * 1e-10); the loop ends when max |d| < 5e-5;
//   * the trial inverse pose is M(d) * invM, M(d) the rigid motion of translation d[0..2] and MRP rotation d[3..5]; accepted when its
//     energy is below the current one (lambda * 0.1; the loop ends when the relative decrease is below 1e-4), else lambda * 10 and
//     another step from the same Hessian;
//   * at the end pose_d = invM^-1, coerced (SetInvM, Coerce).
// Precision: the 6x6 solve is in double (se3::solve_spd), the pose update and the energies in float.  The kernels read the pose as a
// float matrix, and the accept test compares float energies as the reference does, so keeping invM in float follows the reference's
// trajectory most closely; the solve in double only removes the rounding of a float Cholesky from the step.
// Every evaluation returns the energy together with the gradient and Hessian at the same pose (one pass over the points): the
// reference asks for them once a step is accepted, at exactly that pose, which the loop then uses without a second pass.
#pragma once

#include <cmath>
#include <cstring>

#include "../../include/itm_hip.h"
#include "se3.h"

namespace itm {

struct RenPoint {             // one evaluation: energy, gradient, Hessian (hessian[r + c * 6]) at a float inverse pose
  float invM[16];
  float f = 0.0f;
  float g[6] = {0, 0, 0, 0, 0, 0};
  float H[36] = {};
};

constexpr int kRenMaxSteps = 100;
constexpr float kRenMinStep = 0.00005f;
constexpr float kRenMinDecrease = 0.0001f;
constexpr float kRenRegionIncrease = 0.10f;
constexpr float kRenRegionDecrease = 10.0f;

// rotation of the modified Rodrigues parameters r (row-major R: x_out = R x_in)
inline void ren_mrp_rotation(const float* r, float* R) {
  const float a = r[0], b = r[1], c = r[2];
  const float s = a * a + b * b + c * c;
  const float u = 1 - s;
  R[0] = 4 * a * a - 4 * b * b - 4 * c * c + u * u; R[1] = 8 * a * b - 4 * c * u;                  R[2] = 8 * a * c + 4 * b * u;
  R[3] = 8 * a * b + 4 * c * u;                  R[4] = 4 * b * b - 4 * a * a - 4 * c * c + u * u; R[5] = 8 * b * c - 4 * a * u;
  R[6] = 8 * a * c - 4 * b * u;                  R[7] = 8 * b * c + 4 * a * u;                  R[8] = 4 * c * c - 4 * b * b - 4 * a * a + u * u;
  const float den = (1 + s) * (1 + s);
  for (int i = 0; i < 9; ++i) R[i] /= den;
}

// the step as a column-major matrix (ORUtils::Matrix4 storage, m[col * 4 + row]): rotation R, translation step[0..2]
inline void ren_step_matrix(const float* step, float* M) {
  float R[9];
  ren_mrp_rotation(step + 3, R);
  for (int c = 0; c < 3; ++c) {
    for (int r = 0; r < 3; ++r) M[4 * c + r] = R[3 * r + c];
    M[4 * c + 3] = 0.0f;
  }
  M[12] = step[0]; M[13] = step[1]; M[14] = step[2]; M[15] = 1.0f;
}

// column-major 4x4 product lhs * rhs, each element accumulated from zero over k (ORUtils::Matrix4::operator*)
inline void ren_matmul4(const float* lhs, const float* rhs, float* out) {
  for (int x = 0; x < 4; ++x)
    for (int y = 0; y < 4; ++y) {
      float r = 0.0f;
      for (int k = 0; k < 4; ++k) r += lhs[k * 4 + y] * rhs[x * 4 + k];
      out[x * 4 + y] = r;
    }
}

// ComputeSingleStep: -(H + damping)^-1 g, in double
inline void ren_step(const RenPoint& x, float lambda, float step[6]) {
  double A[36], b[6], d[6];
  for (int i = 0; i < 36; ++i) A[i] = (double)x.H[i];
  for (int i = 0; i < 6; ++i) {
    b[i] = (double)x.g[i];
    double& a = A[i * 7];
    if (!(std::fabs(x.H[i * 7]) < 1e-15f)) a = (double)(x.H[i * 7] * (1.0f + lambda));
    else a = (double)(lambda * 1e-10f);
  }
  se3::solve_spd(A, 6, 6, b, d);          // symmetric: the column-major layout reads the same as row-major
  for (int i = 0; i < 6; ++i) step[i] = -(float)d[i];
}

// `evaluate(x)` fills x.f / g / H at x.invM (0 = ok).  M_d_in: pose_d on entry; writes the coerced pose_d.
template <class Evaluate>
inline int ren_track(const float M_d_in[16], float M_d_out[16], Evaluate&& evaluate, int* evaluations) {
  *evaluations = 0;
  se3::Rigid inv;
  if (!se3::invert(se3::from_matrix(M_d_in), inv)) return ITM_ERR_INVALID;
  RenPoint x, x2;
  se3::to_matrix(inv, x.invM);
  int rc = evaluate(x);
  ++*evaluations;
  if (rc) return rc;
  float lambda = 1000.0f;
  bool converged = false;
  for (int iter = 0; iter < kRenMaxSteps && !converged; ++iter) {
    for (;;) {
      float step[6], D[16];
      ren_step(x, lambda, step);
      float maxNorm = 0.0f;
      for (int i = 0; i < 6; ++i) maxNorm = std::fmax(maxNorm, std::fabs(step[i]));
      if (maxNorm < kRenMinStep) { converged = true; break; }
      ren_step_matrix(step, D);
      ren_matmul4(D, x.invM, x2.invM);
      rc = evaluate(x2);
      ++*evaluations;
      if (rc) return rc;
      if (x2.f < x.f) {
        if (std::fabs(x2.f - x.f) / std::fabs(x.f) < kRenMinDecrease) converged = true;
        lambda *= kRenRegionIncrease;
        x = x2;
        break;
      }
      lambda *= kRenRegionDecrease;
    }
  }
  // SetInvM + Coerce: the inverse of invM, projected onto a rigid motion
  se3::Rigid M;
  if (!se3::invert(se3::from_matrix(x.invM), M)) return ITM_ERR_INVALID;
  se3::to_matrix(se3::exp(se3::log(M)), M_d_out);
  return ITM_OK;
}

}  // namespace itm
