// align_solver.h -- host side of the scene aligner (include/itm_hip.h: itm_aligner_align): the Levenberg-Marquardt loop over the pose
// dstFromSrc, its two steps on their own, the checks of its input and the conditioning of a Hessian.  Plain C++ (no HIP); align.hip
// evaluates cost, gradient and Hessian on the GPU.  The reference has no counterpart.
//
//   * the pose is an se3::Rigid in double and is rounded to float once per evaluation (the kernel reads a float matrix);
//   * a step solves (H + lambda diag(H)) step = -nabla in double (se3::solve_spd; a diagonal entry below 1e-15 replaced by
//     lambda * 1e-10, as ren_step does); the trial pose is exp(step) o pose, the twist on the left;
//   * a trial is accepted when it has enough valid samples and a smaller MEAN cost (the valid set changes with the pose, raw sums
//     do not compare): lambda * 0.1, else lambda * 10; a system that is not positive definite is a rejected step without an evaluation;
//   * the loop ends on the step size alone (max |step| < minStep), on lambda > 1e8 or on the evaluation budget: no relative-decrease
//     test, so the last iterate lies within about a step of the fixed point;
//   * conditioning: the smallest eigenvalue of S H S, S = diag(a, a, a, b, b, b) with 1 / a^2 the largest translational and 1 / b^2 the
//     largest rotational diagonal entry of H: free of the two units (metres, radians) and of nothing else.  Scaling every parameter
//     by its own diagonal entry would also hide a parameter that nothing constrains: a rotation about a coordinate axis that is an
//     axis of symmetry of the scene has a diagonal entry made of discretisation noise alone, which such a scaling turns into a 1.
#pragma once

#include <cmath>
#include <cstring>

#include "../../include/itm_hip.h"
#include "se3.h"

namespace itm {

constexpr double kAlignLambdaStart = 1.0;
constexpr double kAlignLambdaMax = 1e8;
constexpr double kAlignAccept = 0.1, kAlignReject = 10.0;

// nullptr when the matrix and the configuration are what itm_aligner_evaluate / itm_aligner_align take, else the reason
inline const char* align_refusal(const float M[16], const itm_align_config& cfg) {
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(M[i])) return "the matrix has an entry that is not finite";
  const se3::Rigid g = se3::from_matrix(M);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double d = g.R[i] * g.R[j] + g.R[3 + i] * g.R[3 + j] + g.R[6 + i] * g.R[6 + j] - (i == j ? 1.0 : 0.0);
      if (!(std::fabs(d) <= 1e-3)) return "the linear part is not orthonormal (an entry of R^T R - I above 1e-3)";
    }
  const double* R = g.R;
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0.0) return "the linear part is a reflection (det R < 0)";
  if (!(cfg.huberDelta > 0.0f)) return "huberDelta is not positive";
  if (!(cfg.minStep > 0.0f)) return "minStep is not positive";
  return nullptr;
}

// the rotation next to a nearly orthonormal matrix: three steps of R <- R (3 I - R^T R) / 2 (each squares the distance; an
// orthonormal matrix stays bit for bit), as itm_rigid_quantise takes them
inline void align_orthonormalise(se3::Rigid& g) {
  for (int step = 0; step < 3; ++step) {
    double G[9], N[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[3 * i + j] = (i == j ? 3.0 : 0.0) - (g.R[i] * g.R[j] + g.R[3 + i] * g.R[3 + j] + g.R[6 + i] * g.R[6 + j]);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) N[3 * i + j] = 0.5 * (g.R[3 * i] * G[j] + g.R[3 * i + 1] * G[3 + j] + g.R[3 * i + 2] * G[6 + j]);
    memcpy(g.R, N, sizeof N);
  }
}

// -(H + lambda diag(H))^-1 nabla in double; false (step = 0) when the damped system is not positive definite
inline bool align_step(const itm_align_eval& e, double lambda, double step[6]) {
  double A[36], b[6];
  for (int i = 0; i < 36; ++i) A[i] = (double)e.hessian[i];
  for (int i = 0; i < 6; ++i) {
    b[i] = -(double)e.nabla[i];
    const double d = (double)e.hessian[i * 7];
    A[i * 7] = !(std::fabs(d) < 1e-15) ? d + lambda * d : lambda * 1e-10;
  }
  return se3::solve_spd(A, 6, 6, b, step);      // symmetric: the column-major layout reads the same as row-major
}

inline se3::Rigid align_apply(const se3::Rigid& pose, const double step[6]) {
  se3::Twist x;
  for (int i = 0; i < 3; ++i) { x.v[i] = step[i]; x.w[i] = step[3 + i]; }
  return se3::compose(se3::exp(x), pose);
}

// Smallest eigenvalue of S H S, H = hessian[r + c * 6], S = diag(a, a, a, b, b, b) with a = 1 / sqrt(max H_kk, k < 3) and
// b = 1 / sqrt(max H_kk, k >= 3): cyclic Jacobi sweeps in double.  0 when a block has no positive diagonal entry.
inline double align_conditioning(const float hessian[36]) {
  double a[36], s[6];
  for (int b = 0; b < 2; ++b) {
    double d = 0.0;
    for (int i = 3 * b; i < 3 * b + 3; ++i) d = std::fmax(d, (double)hessian[i * 7]);
    if (!(d > 0.0) || !std::isfinite(d)) return 0.0;
    for (int i = 3 * b; i < 3 * b + 3; ++i) s[i] = 1.0 / std::sqrt(d);
  }
  for (int r = 0; r < 6; ++r)
    for (int c = 0; c < 6; ++c) a[6 * r + c] = 0.5 * ((double)hessian[r + c * 6] + (double)hessian[c + r * 6]) * s[r] * s[c];
  for (int sweep = 0; sweep < 50; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) off += a[6 * p + q] * a[6 * p + q];
    if (off < 1e-30) break;
    for (int p = 0; p < 6; ++p)
      for (int q = p + 1; q < 6; ++q) {
        const double apq = a[6 * p + q];
        if (apq == 0.0) continue;
        const double theta = (a[6 * q + q] - a[6 * p + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < 6; ++k) {      // columns p and q
          const double akp = a[6 * k + p], akq = a[6 * k + q];
          a[6 * k + p] = c * akp - sn * akq;
          a[6 * k + q] = sn * akp + c * akq;
        }
        for (int k = 0; k < 6; ++k) {      // rows p and q
          const double apk = a[6 * p + k], aqk = a[6 * q + k];
          a[6 * p + k] = c * apk - sn * aqk;
          a[6 * q + k] = sn * apk + c * aqk;
        }
      }
  }
  double lo = a[0];
  for (int i = 1; i < 6; ++i) lo = a[7 * i] < lo ? a[7 * i] : lo;
  return lo;
}

inline double align_mean_cost(const itm_align_eval& e) { return e.noValid > 0 ? (double)e.f / (double)e.noValid : 0.0; }

// `evaluate(M, e)` fills e at the float matrix M (0 = ok).  in / out: dstFromSrc, column-major.  The input has passed align_refusal.
template <class Evaluate>
inline int align_run(const float in[16], const itm_align_config& cfg, Evaluate&& evaluate, float out[16], itm_align_result* res) {
  itm_align_result r;
  memset(&r, 0, sizeof r);
  se3::Rigid pose = se3::from_matrix(in);
  align_orthonormalise(pose);
  float M[16];
  itm_align_eval cur, trial;
  se3::to_matrix(pose, M);
  int rc = evaluate(M, cur);
  if (rc) return rc;
  r.evaluations = 1;
  r.noValid = cur.noValid;
  r.initialCost = r.finalCost = align_mean_cost(cur);
  if (cur.noValid < cfg.minValid || cur.noValid <= 0) {
    r.status = ITM_ALIGN_TOO_FEW_SAMPLES;
    memcpy(out, in, 16 * sizeof(float));
    if (res) *res = r;
    return ITM_OK;
  }
  double lambda = kAlignLambdaStart;
  r.status = ITM_ALIGN_MAX_EVALUATIONS;
  while (r.evaluations < cfg.maxEvaluations) {
    double step[6];
    bool accepted = false;
    if (align_step(cur, lambda, step)) {
      double largest = 0.0;
      for (int i = 0; i < 6; ++i) largest = std::fmax(largest, std::fabs(step[i]));
      if (largest < (double)cfg.minStep) { r.status = ITM_ALIGN_CONVERGED; break; }
      const se3::Rigid next = align_apply(pose, step);
      se3::to_matrix(next, M);
      rc = evaluate(M, trial);
      if (rc) return rc;
      ++r.evaluations;
      accepted = trial.noValid >= cfg.minValid && trial.noValid > 0 && align_mean_cost(trial) < align_mean_cost(cur);
      if (accepted) { pose = next; cur = trial; lambda *= kAlignAccept; }
    }
    if (!accepted) {
      lambda *= kAlignReject;
      if (lambda > kAlignLambdaMax) { r.status = ITM_ALIGN_STALLED; break; }
    }
  }
  r.noValid = cur.noValid;
  r.finalCost = align_mean_cost(cur);
  r.conditioning = align_conditioning(cur.hessian);
  if (r.conditioning < (double)cfg.minConditioning) r.status = ITM_ALIGN_DEGENERATE;
  se3::to_matrix(pose, out);
  if (res) *res = r;
  return ITM_OK;
}

}  // namespace itm
