// The moments of |ifft(H_LS)|^2 that MMSE_CE.m:19-24 takes from h = ifft(H_est_LS) (Main_model_Task_5.m:178-180), as
// Hermitian forms on the Np pilot LS values y of a frame.  H_LS = W y with W the real [N_carrier x Np] operator of interpolate.m
// (spline_op.hpp), so h = B y with B = ifft of W's columns and
//   sum_k k^q |h_k|^2 = y^H A_q y,   A_q(i, j) = sum_k k^q conj(B(k, i)) B(k, j),   q = 0, 1, 2,   k = 0 .. N_carrier - 1:
// 3 Np^2 multiply-adds per frame instead of an N_carrier-point transform.  Built once per plan, in double.
// Host code only, no device or library dependency: the stand-alone check of tests/test_mmse_ls_host.py compiles it alone.
#pragma once
#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ofdm {

using ls_zc = std::complex<double>;

// out[k] = sum_t x[t * stride] root[(k t N / n) mod N], n | N: mixed-radix decimation in time, any n (a prime factor p costs p per point)
inline void ls_dft_rec(const ls_zc* x, size_t stride, ls_zc* out, int n, const std::vector<ls_zc>& root, int N) {
  if (n == 1) { out[0] = x[0]; return; }
  int p = 2;
  while (n % p != 0) p = (p * p > n) ? n : p + 1;
  const int m = n / p;
  const int64_t step = N / n;
  for (int r = 0; r < p; ++r) ls_dft_rec(x + (size_t)r * stride, stride * (size_t)p, out + (size_t)r * m, m, root, N);
  std::vector<ls_zc> t(p), u(p);
  for (int k = 0; k < m; ++k) {
    for (int r = 0; r < p; ++r) t[r] = out[(size_t)r * m + k] * root[(size_t)(((int64_t)r * k * step) % N)];
    for (int s = 0; s < p; ++s) {
      ls_zc acc(0, 0);
      for (int r = 0; r < p; ++r) acc += t[r] * root[(size_t)(((int64_t)r * s * m * step) % N)];
      u[s] = acc;
    }
    for (int s = 0; s < p; ++s) out[(size_t)s * m + k] = u[s];
  }
}

// W [nc x np] column-major (build_interpolate_operator) -> A [3][np][np]: A_q(i, j) at q * np * np + j * np + i
inline void build_ls_moment_forms(const double* W, int nc, int np, std::vector<ls_zc>& A) {
  const long double two_pi = 6.283185307179586476925286766559005768L;
  std::vector<ls_zc> root(nc);                                        // exp(+2 pi i t / nc): the inverse transform
  for (int t = 0; t < nc; ++t) {
    const long double a = two_pi * (long double)t / (long double)nc;
    root[t] = ls_zc((double)cosl(a), (double)sinl(a));
  }
  std::vector<ls_zc> B((size_t)np * nc), col(nc);                    // B [np][nc]: column j of ifft(W), contiguous in k
  for (int j = 0; j < np; ++j) {
    for (int m = 0; m < nc; ++m) col[m] = ls_zc(W[m + (size_t)j * nc], 0.0);
    ls_dft_rec(col.data(), 1, &B[(size_t)j * nc], nc, root, nc);
    for (int k = 0; k < nc; ++k) B[(size_t)j * nc + k] /= (double)nc;
  }
  const size_t plane = (size_t)np * np;
  A.assign(3 * plane, ls_zc(0, 0));
  for (int i = 0; i < np; ++i)
    for (int j = i; j < np; ++j) {                                    // Hermitian: A_q(j, i) = conj(A_q(i, j))
      const ls_zc *bi = &B[(size_t)i * nc], *bj = &B[(size_t)j * nc];
      double s0r = 0, s0i = 0, s1r = 0, s1i = 0, s2r = 0, s2i = 0;
      for (int k = 0; k < nc; ++k) {
        const double pr = bi[k].real() * bj[k].real() + bi[k].imag() * bj[k].imag();     // conj(bi) * bj
        const double pi = bi[k].real() * bj[k].imag() - bi[k].imag() * bj[k].real();
        const double kk = (double)k;
        s0r += pr; s0i += pi;
        s1r += pr * kk; s1i += pi * kk;
        s2r += pr * kk * kk; s2i += pi * kk * kk;
      }
      const ls_zc s[3] = {ls_zc(s0r, s0i), ls_zc(s1r, s1i), ls_zc(s2r, s2i)};
      for (int q = 0; q < 3; ++q) {
        A[q * plane + (size_t)j * np + i] = s[q];
        A[q * plane + (size_t)i * np + j] = i == j ? ls_zc(s[q].real(), 0.0) : std::conj(s[q]);
      }
    }
}

}  // namespace ofdm
