// The register scans behind every power-of-two window of calculate_window_PAPR.m:8-14: the body window_papr_reg_kernel
// (ofdm_papr.hip, one double per window to HBM) and papr_hist_kernel (ofdm_papr_study.hip, one count per window in LDS) share.
#pragma once

#include <limits>

#include "ofdm_common.hpp"

namespace ofdm {

__device__ __forceinline__ int lds_pad(int j) { return j + (j >> 5); }        // 1 double per 32: chunked scans stay conflict-free

template <typename T>
__device__ __forceinline__ double power_of(cx<T> v) { return (double)v.x * (double)v.x + (double)v.y * (double)v.y; }

__device__ __forceinline__ double wave_excl_sum(double v, int lane) {
  double inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  return inc - v;
}
__device__ __forceinline__ double wave_excl_max(double v, int lane) {       // identity 0: all values are powers >= 0
  double inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const double o = __shfl_up(inc, d, 64);
    if (lane >= d) inc = fmax(inc, o);
  }
  const double prev = __shfl_up(inc, 1, 64);
  return lane ? prev : 0.0;
}

// Every window start base + r, r < W, of the n samples x[0 .. n) with base + r < n_out, for a whole workgroup of 2 W / C threads.
// The first half of the workgroup owns the first block mirrored (q <-> sample W-1-q), the second half the second block
// (q <-> sample W+q), C = 2 W / threads consecutive q per thread; a prefix scan over q is then the suffix scan the first block
// needs and the prefix scan the second one needs.  Window r = max / sum of suffix(first block, r) and prefix(second block, r-1):
// no subtraction of large prefix sums.  LDS only carries the coalesced load (chunks are read back conflict-free through lds_pad)
// and the finished scans; TWO_PHASE (W = 8192) reuses one pair of arrays for the maxima and then the sums.
//   a: (TWO_PHASE ? 2 : 4) * (W + W / 32 + 1) doubles of LDS; wtot_m, wtot_s: 16 doubles of LDS each
//   emit(i, v): window start i of the signal and its value 10 log10(max / mean) (calculatePAPR.m:4-10), NaN for an all-zero window
//   seen(sample): every sample the thread loaded (zeros beyond the signal's end), once
template <typename T, int C, bool TWO_PHASE, typename Emit, typename Seen>
__device__ __forceinline__ void window_papr_scan(const cx<T>* __restrict__ x, int64_t n, int W, int64_t base, int64_t n_out,
                                                 double* __restrict__ a, double* __restrict__ wtot_m, double* __restrict__ wtot_s,
                                                 Emit emit, Seen seen) {
  const int nt = blockDim.x, half = nt >> 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = tid >= half, u = tid - blk * half;
  const int wp = W + (W >> 5) + 1;
  double* const M = a;                                // [2][wp]
  double* const S = TWO_PHASE ? a : a + 2 * wp;       // [2][wp]
  cx<T> xv[C];                                        // all C loads of a thread in flight together
#pragma unroll
  for (int e = 0; e < C; ++e) {
    const int64_t g = base + tid + e * nt;
    xv[e] = g < n ? x[g] : mk<T>(0, 0);
  }
#pragma unroll
  for (int e = 0; e < C; ++e) {
    seen(xv[e]);
    const int j = tid + e * nt;
    const int b = j >= W, q = b ? j - W : W - 1 - j;
    M[b * wp + lds_pad(q)] = power_of(xv[e]);
  }
  __syncthreads();
  double m[C], s[C];
  double mrun = 0.0, srun = 0.0;
#pragma unroll
  for (int e = 0; e < C; ++e) {
    const double p = M[blk * wp + lds_pad(u * C + e)];
    mrun = fmax(mrun, p);
    srun += p;
    m[e] = mrun;
    s[e] = srun;
  }
  double em = wave_excl_max(mrun, lane), es = wave_excl_sum(srun, lane);
  if (lane == 63) { wtot_m[wave] = fmax(em, mrun); wtot_s[wave] = es + srun; }
  __syncthreads();                                    // also: every chunk has been read, M may be overwritten
  for (int w = blk * (half >> 6); w < wave; ++w) { em = fmax(em, wtot_m[w]); es += wtot_s[w]; }
#pragma unroll
  for (int e = 0; e < C; ++e) {
    M[blk * wp + lds_pad(u * C + e)] = fmax(m[e], em);
    if (!TWO_PHASE) S[blk * wp + lds_pad(u * C + e)] = s[e] + es;
  }
  __syncthreads();
  constexpr int NOUT = C / 2;                         // W / threads
  double mx[NOUT];
#pragma unroll
  for (int k = 0; k < NOUT; ++k) {
    const int r = tid + k * nt;
    mx[k] = M[lds_pad(W - 1 - r)];
    if (r) mx[k] = fmax(mx[k], M[wp + lds_pad(r - 1)]);
  }
  if (TWO_PHASE) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < C; ++e) S[blk * wp + lds_pad(u * C + e)] = s[e] + es;
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NOUT; ++k) {
    const int r = tid + k * nt;
    if (base + r < n_out) {
      double sum = S[lds_pad(W - 1 - r)];
      if (r) sum += S[wp + lds_pad(r - 1)];
      const double v = 10.0 * log10(mx[k] / (sum / (double)W));          // calculatePAPR.m:4-10
      emit(base + r, v == v ? v : std::numeric_limits<double>::quiet_NaN());
    }
  }
}

}  // namespace ofdm
