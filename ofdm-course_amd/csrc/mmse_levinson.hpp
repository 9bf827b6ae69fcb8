// MMSE_CE.m:25-36 for one frame per WAVEFRONT (shared by mmse_wave_kernel of ofdm_part2.hip and mmse_ls_wave_kernel of
// ofdm_chain_mmse_ls.hip): Rpp = rf2 + I/snr is Hermitian Toeplitz with first column 1/(1 + j c k), c = 2 pi tau_rms df Nps;
// z = Rpp \ H_tilde by the Levinson recursion in double, all state in wave-private LDS, no workgroup barrier;
// out = rf2 * z (the first Np rows of Rhp/Rpp*H_tilde, which is all MMSE_CE.m:38 keeps).
#pragma once
#include "chain_fast_core.hpp"

namespace ofdm {

__device__ __forceinline__ double p2_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// y: the frame's Np pilot LS values; tcol: 4 * np c64 of wave-private LDS (tcol, fv, bv, xv); vout: the frame's Np outputs
template <typename T>
__device__ __forceinline__ void mmse_toeplitz_wave(const cx<T>* __restrict__ y, double c, double inv_snr, int np, c64* tcol,
                                                   cx<T>* __restrict__ vout, int lane) {
  c64 *fv = tcol + np, *bv = fv + np, *xv = bv + np;
  for (int k = lane; k < np; k += 64) {
    const double d = 1.0 + (c * k) * (c * k);
    tcol[k] = c64{1.0 / d, -(c * k) / d};
  }
  wave_sync();
  const double t0 = tcol[0].x + inv_snr;
  if (lane == 0) {
    fv[0] = c64{1.0 / t0, 0};
    bv[0] = c64{1.0 / t0, 0};
    xv[0] = c64{(double)y[0].x / t0, (double)y[0].y / t0};
  }
  wave_sync();
  for (int n = 1; n < np; ++n) {
    // eps_f = sum_i T[n][i] f[i], eps_x = sum_i T[n][i] x[i], eps_b = sum_i T[0][i+1] b[i],  i < n   (T[i][j] = t(i - j))
    c64 ef{0, 0}, ex{0, 0}, eb{0, 0};
    for (int i = lane; i < n; i += 64) {
      const c64 tn = tcol[n - i];
      ef = ef + tn * fv[i];
      ex = ex + tn * xv[i];
      eb = eb + conj(tcol[i + 1]) * bv[i];
    }
    ef = c64{p2_wave_sum(ef.x), p2_wave_sum(ef.y)};
    ex = c64{p2_wave_sum(ex.x), p2_wave_sum(ex.y)};
    eb = c64{p2_wave_sum(eb.x), p2_wave_sum(eb.y)};
    const c64 one{1, 0};
    const c64 inv = cdiv(one, one - eb * ef);
    const c64 dx = c64{(double)y[n].x, (double)y[n].y} - ex;
    // new f = inv [f; 0] - ef inv [0; b] ; new b = inv [0; b] - eb inv [f; 0] ; x += dx * new b.  Entry i reads the old f[i]
    // and b[i - 1] and writes index i: 64-entry chunks from the top down, each chunk reading before it writes, never
    // overwrite an input of a chunk still to come.
    for (int i0 = (n / 64) * 64; i0 >= 0; i0 -= 64) {
      const int i = i0 + lane;
      c64 nf{0, 0}, nb{0, 0}, nx{0, 0};
      if (i <= n) {
        const c64 fe = (i < n) ? fv[i] : c64{0, 0};
        const c64 be = (i > 0) ? bv[i - 1] : c64{0, 0};
        nf = inv * fe - (ef * inv) * be;
        nb = inv * be - (eb * inv) * fe;
        nx = ((i < n) ? xv[i] : c64{0, 0}) + dx * nb;
      }
      wave_sync();
      if (i <= n) {
        fv[i] = nf;
        bv[i] = nb;
        xv[i] = nx;
      }
      wave_sync();
    }
  }
  // ---- out = rf2 * z (no 1/snr on this diagonal)
  for (int i = lane; i < np; i += 64) {
    c64 acc{0, 0};
    for (int j = 0; j < np; ++j) {
      const int k = i - j;
      const c64 t = k >= 0 ? tcol[k] : conj(tcol[-k]);
      acc = acc + t * xv[j];
    }
    vout[i] = mk<T>((T)acc.x, (T)acc.y);
  }
}

}  // namespace ofdm
