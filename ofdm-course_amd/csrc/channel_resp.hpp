// The true channel of a generated frame on carrier k: H_f(k) = sum_t a_{f,t} e^{-2 pi i d_t k / Nfft} = fft(h_f, Nfft)(k) of
// get_MP_channel_resp (T5/Task5_part2.m:160-166), in double.  One definition for the per-frame error sum of the sweeps
// (t5_frame_nmse_kernel, ofdm_ber_sweep.hip) and the per-carrier profile of the channel study (ofdm_hest_study.hip), so both see
// the same H.
#pragma once

#include "ofdm_common.hpp"
#include "txf_plan.hpp"

namespace ofdm {

// the delays of a channel's taps (a kernel argument); the amplitudes are device memory
struct TxfDelays {
  int32_t d[TXF_MAX_TAPS];
  int n;
};

// a: the frame's dl.n amplitudes; inv = 2 / Nfft.  The phase d_t k mod Nfft is reduced in integers, so the argument of sincospi
// stays in [0, 2).  The taps are added in index order.
__device__ __forceinline__ void channel_resp(const c64* a, const TxfDelays& dl, int k, int nfft, double inv, double& hr, double& hi) {
  hr = 0;
  hi = 0;
  for (int t = 0; t < dl.n; ++t) {
    const int m = (int)(((int64_t)dl.d[t] * k) % nfft);       // the phase reduced in integers: the argument stays in [0, 2)
    double sn, cs;
    sincospi((double)m * inv, &sn, &cs);
    hr += a[t].x * cs + a[t].y * sn;                           // a (cs - i sn)
    hi += a[t].y * cs - a[t].x * sn;
  }
}

}  // namespace ofdm
