// One carrier of one frame, the true H against an estimate: what the channel study (ofdm_hest_study.hip) and the estimator profile
// (ofdm_est_profile.hip) sum per carrier.  Device code, included by the study .hip files only.
#pragma once

#include "ofdm_common.hpp"

namespace ofdm {

// sqrt(re^2 + im^2) as two rounded products, a rounded sum and a root, never a fused operation: what a host that rebuilds the value
// from H_est computes (the build contracts in the backend, where a pragma does not reach: the products pass through an empty asm)
__device__ __forceinline__ double hest_abs(double re, double im) {
  double p = re * re, q = im * im;
  asm volatile("" : "+v"(p), "+v"(q));
  return sqrt(p + q);
}

// one carrier (or pilot) of one frame: the true H against the estimate e
struct HestPoint {
  double est_amp, true_amp, err, amp_err;
  uint8_t bad;
};

template <typename T>
__device__ __forceinline__ HestPoint hest_point(double hr, double hi, cx<T> e) {
  const double er = (double)e.x, ei = (double)e.y;
  HestPoint p;
  p.bad = (er - er == 0.0 && ei - ei == 0.0) ? 0 : 1;
  p.est_amp = hest_abs(er, ei);
  p.true_amp = hest_abs(hr, hi);
  const double dr = hr - er, di = hi - ei, d = p.est_amp - p.true_amp;
  p.err = dr * dr + di * di;
  p.amp_err = d * d;
  return p;
}

}  // namespace ofdm
