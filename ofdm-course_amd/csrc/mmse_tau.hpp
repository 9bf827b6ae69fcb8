// The rms delay spread of MMSE_CE.m:19-24 from the three moments of |h_k|^2,
//   s0 = sum |h_k|^2,  s1 = sum |h_k|^2 k,  s2 = sum |h_k|^2 k^2:   tau_rms = sqrt(s2 / s0 - (s1 / s0)^2),
// and the factor c = 2 pi tau_rms df Nps of the correlation 1 / (1 + j c (i - j)) (:25-26, :30, :33).
// When all the energy of h sits in one bin the exact difference is 0 and the computed one is rounding noise of either sign
// (about one (amplitude, delay) pair in seven comes out negative).  MMSE_CE.m takes a complex square root there and goes on with
// tau ~ 1e-8 i; a real sqrt would hand NaN to every carrier.  The difference is clamped at 0, the exact value of that corner.
// Every MMSE entry of the library takes tau_rms from here, so the rule exists once.  s0 = 0 (no energy at all) is the caller's
// to refuse: fmax drops the NaN of 0 / 0 and tau comes out 0.
// No device or library dependency: the stand-alone check of tests/test_mmse_tau_host.py compiles it alone.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define OFDM_TAU_HD __host__ __device__
#else
#define OFDM_TAU_HD
#endif

namespace ofdm {

// tau_rms (MMSE_CE.m:20-24)
OFDM_TAU_HD inline double mmse_tau_rms(double s0, double s1, double s2) {
  const double r = s1 / s0, r2 = s2 / s0;
  return sqrt(fmax(r2 - r * r, 0.0));
}

// c = 2 pi tau_rms df Nps (:25-26, :30)
OFDM_TAU_HD inline double mmse_tau_c(double s0, double s1, double s2, double df, double nps) {
  return 2.0 * M_PI * mmse_tau_rms(s0, s1, s2) * df * nps;
}

}  // namespace ofdm
