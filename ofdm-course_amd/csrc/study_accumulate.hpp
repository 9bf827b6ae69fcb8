// The accumulate stage of the spectrum, sync, fine and IFO studies: device code, included by the study .hip files only.  A chunk's
// rows [nf][cols] of doubles are added into the point's accumulators [cols], and a chunk's per-frame scalars [nf] into a pair of
// sums.  The launch shape is txf_plan.hpp's STUDY_ACC_*: workgroups of 256 threads own 64 columns each; where a study has scalars,
// one more workgroup, the last, takes them.
//
// The sum of a column is one chain of additions -- sums[k] = (..(sums[k] + v_0[k]) + v_1[k]) + .. in frame order, and the chunks of a
// point run in stream order on accumulators the call zeroed, so every double is ((0 + v_0) + v_1) + .. whatever the chunking -- so
// the loads are what can overlap: the four wavefronts stage STUDY_ACC_TILE rows at a time in LDS (sixteen loads in flight per thread,
// 512 bytes per wavefront and row), then wavefront 0 adds the tile to its columns in frame order.  What does not depend on the order
// -- a peak by fmax, a count by + -- every thread folds over the rows it loaded, and the four row groups' partials meet in the tile
// once it is free.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "txf_plan.hpp"      // STUDY_ACC_*

namespace ofdm {

// s + v^2 as a rounded product and a rounded sum, never one fused operation: what a host that rebuilds the sum from the per-frame
// values computes.  The build contracts in the backend (-ffp-contract=fast), where a pragma on the statement does not reach, so
// the product passes through an empty asm statement that the combiner cannot look through.
__device__ __forceinline__ double add_square(double s, double v) {
  double p = v * v;
  asm volatile("" : "+v"(p));
  return s + p;
}

using StudyAccTile = double[STUDY_ACC_TILE][STUDY_ACC_COLS];

// where a column's peak comes from: nowhere, the rows the sum reads, or a second array of the same shape
enum { ACC_PEAK_OFF, ACC_PEAK_ROWS, ACC_PEAK_SECOND };

// The column workgroups.  DROP: a value that is not finite (isfinite; `a - a == 0.0` is the same predicate on every double) is
// counted in dropped[k] and not added; otherwise it is added like any other.  PEAK: peak[k] = fmax(peak[k], the rows' or
// peak_rows' entries), only where `peak` is given.  COUNT: counts[k] += the bytes flags[f][k].  The pointers a switch leaves unused
// may be null.  Column k >= cols of the last workgroup idles (it still meets every barrier).
// The rows come from `load(f, k)`, the value of frame f of the chunk in column k: a chunk's rows in memory (below), or what a study
// forms of its buffers on the way (the estimator profile, ofdm_est_profile.hip).  With DROP, `dropped` may be null: the values left
// out are then not counted.
template <bool DROP, int PEAK, bool COUNT, typename Load>
__device__ __forceinline__ void study_accumulate_columns_from(StudyAccTile& tile, Load load, const double* __restrict__ peak_rows,
                                                              const uint8_t* __restrict__ flags, int64_t nf, int64_t cols,
                                                              double* __restrict__ sums, unsigned long long* __restrict__ dropped,
                                                              double* __restrict__ peak, unsigned long long* __restrict__ counts) {
  static_assert(PEAK == ACC_PEAK_OFF || !COUNT, "one order-free partial goes through the tile");
  constexpr int RW = STUDY_ACC_THREADS / STUDY_ACC_COLS;                     // row groups: 4
  constexpr int PER = STUDY_ACC_TILE / RW;                                   // rows per thread and tile
  const int c = threadIdx.x % STUDY_ACC_COLS, r = threadIdx.x / STUDY_ACC_COLS;
  const int64_t k = (int64_t)blockIdx.x * STUDY_ACC_COLS + c;
  const bool live = k < cols;
  double s = (r == 0 && live) ? sums[k] : 0.0, m = 0.0;
  unsigned long long nd = 0, nc = 0;
  for (int64_t t0 = 0; t0 < nf; t0 += STUDY_ACC_TILE) {
    double v[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t f = t0 + r * PER + i;
      const bool in = live && f < nf;
      v[i] = in ? load(f, k) : 0.0;
      if (PEAK == ACC_PEAK_ROWS) m = fmax(m, v[i]);
      if (PEAK == ACC_PEAK_SECOND && peak && in) m = fmax(m, peak_rows[f * cols + k]);
      if (COUNT) nc += in ? (unsigned long long)flags[f * cols + k] : 0ull;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) tile[r * PER + i][c] = v[i];
    __syncthreads();
    if (r == 0) {
      const int n = (int)(nf - t0 < STUDY_ACC_TILE ? nf - t0 : STUDY_ACC_TILE);
      for (int q = 0; q < n; ++q) {
        const double a = tile[q][c];
        if (!DROP || isfinite(a)) s += a; else ++nd;
      }
    }
    __syncthreads();
  }
  if (r == 0 && live) {
    sums[k] = s;
    if (DROP && dropped) dropped[k] += nd;
  }
  if (PEAK != ACC_PEAK_OFF && peak) {                 // the tile is free again: [RW][STUDY_ACC_COLS] partials
    tile[r][c] = m;
    __syncthreads();
    if (r == 0 && live) {
      double pm = peak[k];
      for (int q = 0; q < RW; ++q) pm = fmax(pm, tile[q][c]);
      peak[k] = pm;
    }
  }
  if (COUNT) {
    unsigned long long* const cnt = (unsigned long long*)&tile[0][0];
    cnt[r * STUDY_ACC_COLS + c] = nc;
    __syncthreads();
    if (r == 0 && live) {
      unsigned long long t = counts[k];
      for (int q = 0; q < RW; ++q) t += cnt[q * STUDY_ACC_COLS + c];
      counts[k] = t;
    }
  }
}

// rows [nf][cols] of doubles in memory
template <bool DROP, int PEAK, bool COUNT>
__device__ __forceinline__ void study_accumulate_columns(StudyAccTile& tile, const double* __restrict__ rows,
                                                         const double* __restrict__ peak_rows, const uint8_t* __restrict__ flags,
                                                         int64_t nf, int64_t cols, double* __restrict__ sums,
                                                         unsigned long long* __restrict__ dropped, double* __restrict__ peak,
                                                         unsigned long long* __restrict__ counts) {
  study_accumulate_columns_from<DROP, PEAK, COUNT>(
      tile, [rows, cols](int64_t f, int64_t k) { return rows[f * cols + k]; }, peak_rows, flags, nf, cols, sums, dropped, peak, counts);
}

// one per-frame scalar into {sum f(v), sum v^2}: f is fabs (an error) or the identity (a signed value)
template <bool SKIP, bool ABS>
__device__ __forceinline__ void study_add_scalar(double v, double& s1, double& s2) {
  if (!SKIP || isfinite(v)) {
    s1 += ABS ? fabs(v) : v;
    s2 = add_square(s2, v);
  }
}

// The tail workgroup.  err [nf], a chunk's errors, into err_sums = {sum |e|, sum e^2} and, with SIGNED, a second column val [nf] into
// val_sums = {sum v, sum v^2}: STUDY_ACC_THREADS frames at a time through the tile, thread 0 adds in frame order.  SKIP: a value that is
// not finite is left out; otherwise it is added like any other (and the sums are NaN from that frame on).
template <bool SKIP, bool SIGNED>
__device__ __forceinline__ void study_accumulate_scalars(StudyAccTile& tile, const double* __restrict__ err, const double* __restrict__ val,
                                                         int64_t nf, double* __restrict__ err_sums, double* __restrict__ val_sums) {
  double* const fe = &tile[0][0];
  double* const fv = fe + STUDY_ACC_THREADS;
  double e1 = err_sums[0], e2 = err_sums[1], v1 = 0.0, v2 = 0.0;
  if (SIGNED) { v1 = val_sums[0]; v2 = val_sums[1]; }
  for (int64_t t0 = 0; t0 < nf; t0 += STUDY_ACC_THREADS) {
    const int64_t f = t0 + threadIdx.x;
    fe[threadIdx.x] = f < nf ? err[f] : 0.0;
    if (SIGNED) fv[threadIdx.x] = f < nf ? val[f] : 0.0;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = (int)(nf - t0 < STUDY_ACC_THREADS ? nf - t0 : STUDY_ACC_THREADS);
      for (int q = 0; q < n; ++q) {
        const double e = fe[q], v = SIGNED ? fv[q] : 0.0;     // both loads in front of the first column's branch
        study_add_scalar<SKIP, true>(e, e1, e2);
        if (SIGNED) study_add_scalar<SKIP, false>(v, v1, v2);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    err_sums[0] = e1; err_sums[1] = e2;
    if (SIGNED) { val_sums[0] = v1; val_sums[1] = v2; }
  }
}

}  // namespace ofdm
