// The estimator profile: the two pictures the Task-5 drivers draw beside their error numbers, summed over the frames of every point
// of the estimator study's sweep -- |H_freq| against |H_est_LS|, |H_est_MMSE|, |H_est_MP|, |H_est_OMP| over the carriers
// (T5/Main_model_Task_5.m:207-231) and |H_tau| against the delays OMP_estimate picked (:238-242) -- with the histogram of the
// frames' error.  ofdm_estimator_profile is the estimator study's call (est_study_run, est_study.hpp: the same frames, the same
// launches in the same order, the same five outputs bit for bit) with three kernels behind each chunk that only read what the
// chunk left behind:
//
//   est_profile_kernel<T>  the studies' column body (study_accumulate.hpp) over the carriers, one quantity per blockIdx.y: the
//                          truth's |H_f(k)|, then of each estimator |H_e,f(k)|, |H_f(k) - H_e,f(k)|^2 and (|H_e,f(k)| - |H_f(k)|)^2
//                          (hest_point, the channel study's).  One thread owns one carrier of one quantity and adds the chunk's
//                          frames in frame order; the values are formed from the body's H buffers and the truth on the way into
//                          the tile, so the reads are coalesced over k and nothing is stored per frame.  A frame whose
//                          frame_nmse[f][e] is not finite (est_reduce_kernel ran before) is left out of the three sums of e: the
//                          rule and the count of nmse_dropped.  No double is added atomically; the chunks of a point run in
//                          stream order on accumulators the call zeroed: ((0 + v_0) + v_1) + .. whatever the chunking.
//   est_delay_kernel       OMP's picks in the plan's tap workspace (int32 / c64 whatever the plan's precision).  One thread owns
//                          one delay k of the dictionary; the chunk's picks, |x| of their coefficients and |a| of the channel's
//                          taps are staged EST_DELAY_FRAMES frames at a time in LDS, and the owner adds the slots that hold k
//                          (frame order, slot order) and the channel tap at delay k in frame order.  The first workgroup also
//                          takes a frame per thread: the number of picks made, the delays in both the true support (d_t < K) and
//                          the distinct picks, in the one only, in the other only (integer atomics), and with want_frames copies
//                          the picks (1-based, 0 = not made) and coefficients out.
//   est_hist_kernel        every frame and estimator of the chunk on the table of linear thresholds (hest_bin, hest_plan.hpp);
//                          a value that is not finite -- the frames of nmse_dropped -- is counted in nmse_nan (integer atomics).
// MP's taps are not here: the tap workspace holds one pursuit at a time and the body turns MP's taps into H before OMP overwrites
// them.  Host side: the checks, the chunk and the launch shapes are est_profile_plan.hpp's.
#include <algorithm>
#include <cmath>
#include <vector>

#include "est_profile_plan.hpp"
#include "est_study.hpp"
#include "hest_point.hpp"
#include "study_accumulate.hpp"

namespace ofdm {

// the accumulators of one point: quantity q of carrier k at sums[q][k]
struct EstProfileSums {
  double* sums[EST_PROFILE_QUANTITIES];
};

template <typename T>
struct EstProfileRows {
  const cx<T>* h[EST_ROWS];
};

template <typename T>
__global__ __launch_bounds__(STUDY_ACC_THREADS) void est_profile_kernel(const c64* __restrict__ htrue, int64_t h_stride, EstProfileRows<T> est,
                                                                       const double* __restrict__ frame_nmse, int64_t nf, int n_carrier,
                                                                       EstProfileSums acc) {
  __shared__ StudyAccTile tile;
  const int q = blockIdx.y;
  if (q == 0) {                                       // the truth: every frame
    study_accumulate_columns_from<false, ACC_PEAK_OFF, false>(
        tile,
        [=](int64_t f, int64_t k) {
          const c64 t = htrue[f * h_stride + k];
          return hest_abs(t.x, t.y);
        },
        nullptr, nullptr, nf, n_carrier, acc.sums[0], nullptr, nullptr, nullptr);
    return;
  }
  const int e = (q - 1) / EST_PROFILE_PER_EST, j = (q - 1) % EST_PROFILE_PER_EST;
  const cx<T>* const h = est.h[e];
  study_accumulate_columns_from<true, ACC_PEAK_OFF, false>(
      tile,
      [=](int64_t f, int64_t k) {
        if (!isfinite(frame_nmse[f * EST_ROWS + e])) return (double)NAN;      // the frame is dropped for e: DROP leaves it out
        const c64 t = htrue[f * h_stride + k];
        const HestPoint p = hest_point<T>(t.x, t.y, h[f * n_carrier + k]);
        return j == 0 ? p.est_amp : j == 1 ? p.err : p.amp_err;
      },
      nullptr, nullptr, nf, n_carrier, acc.sums[q], nullptr, nullptr, nullptr);
}

struct EstDelayOut {
  unsigned long long* pick_hist;     // [K]
  double* tap_amp_sums;              // [K]
  unsigned long long* n_picks_hist;  // [taps + 1]
  double* true_tap_amp_sums;         // [K]
  unsigned long long* true_outside;  // [1]
  unsigned long long* support;       // [3]: hits, misses, false
  int32_t* picks;                    // [nf][taps] or null
  c64* tap_x;                        // [nf][taps] or null
};

__global__ __launch_bounds__(EST_DELAY_THREADS) void est_delay_kernel(const int32_t* __restrict__ tap_idx, const c64* __restrict__ tap_x,
                                                                     int taps, int k_atoms, const c64* __restrict__ amp,
                                                                     int64_t amp_stride, TxfDelays dl, int64_t nf, EstDelayOut o) {
  __shared__ int32_t s_idx[EST_DELAY_FRAMES * CH_MAXT];
  __shared__ double s_ax[EST_DELAY_FRAMES * CH_MAXT];
  __shared__ double s_ta[EST_DELAY_FRAMES * TXF_MAX_TAPS];
  const int tid = threadIdx.x;
  const int k = blockIdx.x * EST_DELAY_THREADS + tid;
  const bool own = k < k_atoms;
  const bool first = blockIdx.x == 0;
  int my_tap = -1, n_in = 0;                          // the channel tap at delay k (the delays are distinct); the taps below K
  for (int t = 0; t < dl.n; ++t) {
    if (dl.d[t] < k_atoms) ++n_in;
    if (own && dl.d[t] == k) my_tap = t;
  }
  double s = own ? o.tap_amp_sums[k] : 0.0, ts = own ? o.true_tap_amp_sums[k] : 0.0;
  unsigned long long cnt = 0;
  for (int64_t t0 = 0; t0 < nf; t0 += EST_DELAY_FRAMES) {
    const int n = (int)(nf - t0 < EST_DELAY_FRAMES ? nf - t0 : EST_DELAY_FRAMES);
    for (int i = tid; i < n * taps; i += EST_DELAY_THREADS) {
      const int32_t idx = tap_idx[t0 * taps + i];
      const c64 x = tap_x[t0 * taps + i];
      s_idx[i] = idx;
      s_ax[i] = hest_abs(x.x, x.y);
      if (first && o.picks) o.picks[t0 * taps + i] = idx + 1;
      if (first && o.tap_x) o.tap_x[t0 * taps + i] = x;
    }
    for (int i = tid; i < n * dl.n; i += EST_DELAY_THREADS) {
      const c64 a = amp[(t0 + i / dl.n) * amp_stride + i % dl.n];
      s_ta[i] = hest_abs(a.x, a.y);
    }
    __syncthreads();
    if (own) {
      // every slot of the tile in frame order and slot order; the LDS reads do not depend on the chain, so they are unrolled in
      // front of it, and a slot that holds another delay is a select, not a branch: the same additions in the same order
#pragma unroll 8
      for (int i = 0; i < n * taps; ++i) {
        const bool mine = s_idx[i] == k;
        const double t = s + s_ax[i];
        s = mine ? t : s;
        cnt += mine ? 1ull : 0ull;
      }
      if (my_tap >= 0)
        for (int f = 0; f < n; ++f) ts += s_ta[f * dl.n + my_tap];
    }
    if (first && tid < n) {                           // a frame per thread: its pick count and its support against the truth's
      const int32_t* const pk = s_idx + tid * taps;
      int made = 0, distinct = 0, hits = 0;
      for (int q = 0; q < taps; ++q) {
        const int idx = pk[q];
        if (idx < 0) continue;
        ++made;
        bool seen = false;
        for (int q2 = 0; q2 < q; ++q2) seen = seen || pk[q2] == idx;
        if (seen) continue;
        ++distinct;
        for (int t = 0; t < dl.n; ++t)
          if (dl.d[t] == idx) { ++hits; break; }
      }
      atomicAdd(o.n_picks_hist + made, 1ull);
      if (hits) atomicAdd(o.support + 0, (unsigned long long)hits);
      if (n_in - hits) atomicAdd(o.support + 1, (unsigned long long)(n_in - hits));
      if (distinct - hits) atomicAdd(o.support + 2, (unsigned long long)(distinct - hits));
    }
    __syncthreads();
  }
  if (own) {
    o.tap_amp_sums[k] = s;
    o.true_tap_amp_sums[k] = ts;
    if (cnt) atomicAdd(o.pick_hist + k, cnt);
  }
  if (first && tid == 0 && dl.n - n_in > 0) atomicAdd(o.true_outside, (unsigned long long)(dl.n - n_in) * (unsigned long long)nf);
}

struct EstHistOut {
  unsigned long long *hist, *below, *above, *nan_count;   // [4][n_bins], [4], [4], [4] of the point
};

__global__ __launch_bounds__(EST_HIST_THREADS) void est_hist_kernel(const double* __restrict__ frame_nmse, int64_t n, const double* __restrict__ thr,
                                                                   int n_bins, EstHistOut o) {
  const int64_t i = (int64_t)blockIdx.x * EST_HIST_THREADS + threadIdx.x;
  if (i >= n) return;
  const int e = (int)(i % EST_ROWS);
  const double v = frame_nmse[i];
  const int b = isfinite(v) ? hest_bin(v, thr, n_bins) : HEST_BIN_NAN;
  atomicAdd(b >= 0 ? o.hist + (int64_t)e * n_bins + b : b == HEST_BIN_BELOW ? o.below + e : b == HEST_BIN_ABOVE ? o.above + e : o.nan_count + e,
            1ull);
}

struct EstProfileOutputs {
  double *true_amp_sums, *est_amp_sums, *err_sums, *amp_err_sums;
  uint64_t *nmse_hist, *nmse_below, *nmse_above, *nmse_nan;
  uint64_t* pick_hist;
  double* tap_amp_sums;
  uint64_t* n_picks_hist;
  double* true_tap_amp_sums;
  uint64_t *true_outside, *support;
  int32_t* picks;
  c64* tap_x;
  bool any() const {
    return true_amp_sums || est_amp_sums || err_sums || amp_err_sums || nmse_hist || nmse_below || nmse_above || nmse_nan || pick_hist ||
           tap_amp_sums || n_picks_hist || true_tap_amp_sums || true_outside || support || picks || tap_x;
  }
};

// the profile's side of est_study_run
struct EstProfileHook : EstStudyHook {
  ofdm_rx_plan* pl;
  HestBins bins;
  const std::vector<double>* thr;
  EstProfileOutputs out_;
  // device side
  double *d_true = nullptr, *d_est = nullptr, *d_err = nullptr, *d_aerr = nullptr, *d_tamp = nullptr, *d_ttamp = nullptr, *d_thr = nullptr;
  unsigned long long *d_hist = nullptr, *d_below = nullptr, *d_above = nullptr, *d_nan = nullptr, *d_pick = nullptr, *d_npk = nullptr,
                     *d_outside = nullptr, *d_supp = nullptr;
  TxfFrameOut<int32_t> f_picks;
  TxfFrameOut<c64> f_x;
  TxfDelays dl{};
  TxfShape shape{};

  int prelude(const TxfCall& c, bool both_channels, const EstWanted& e, TxfChannel& ch, TxfGains& g, TxfWhy& w) override {
    return est_profile_prelude(c, both_channels, e, bins, ch, g, w);
  }
  const char* what() const override { return "estimator_profile"; }
  bool out() const override { return out_.any(); }
  int64_t chunk(const TxfShape& s, const TxfUse& u, int taps, int64_t frames_per_point, int64_t user_cap) override {
    return est_profile_chunk(s, u, taps, frames_per_point, user_cap);
  }
  int tables(Stage& st, size_t np, size_t fpp) override {
    const size_t nc = (size_t)pl->n_carrier, K = (size_t)pl->k_atoms, T = (size_t)pl->taps, nb = (size_t)bins.n;
    OFDM_TRY(txf_table(st, out_.true_amp_sums, np * nc, d_true));
    OFDM_TRY(txf_table(st, out_.est_amp_sums, np * EST_ROWS * nc, d_est));
    OFDM_TRY(txf_table(st, out_.err_sums, np * EST_ROWS * nc, d_err));
    OFDM_TRY(txf_table(st, out_.amp_err_sums, np * EST_ROWS * nc, d_aerr));
    OFDM_TRY(txf_table(st, out_.nmse_hist, np * EST_ROWS * nb, d_hist));
    OFDM_TRY(txf_table(st, out_.nmse_below, np * EST_ROWS, d_below));
    OFDM_TRY(txf_table(st, out_.nmse_above, np * EST_ROWS, d_above));
    OFDM_TRY(txf_table(st, out_.nmse_nan, np * EST_ROWS, d_nan));
    OFDM_TRY(txf_table(st, out_.pick_hist, np * K, d_pick));
    OFDM_TRY(txf_table(st, out_.tap_amp_sums, np * K, d_tamp));
    OFDM_TRY(txf_table(st, out_.n_picks_hist, np * (T + 1), d_npk));
    OFDM_TRY(txf_table(st, out_.true_tap_amp_sums, np * K, d_ttamp));
    OFDM_TRY(txf_table(st, out_.true_outside, np, d_outside));
    OFDM_TRY(txf_table(st, out_.support, np * 3, d_supp));
    OFDM_TRY(f_picks.out(st, out_.picks, np * fpp * T));
    return f_x.out(st, out_.tap_x, np * fpp * T);
  }
  int begin(Stage& st, const TxfDelays& delays, int64_t) override {
    dl = delays;
    shape = txf_shape(pl);
    void* v = nullptr;
    OFDM_TRY(st.scratch(sizeof(double) * thr->size(), &v));
    d_thr = (double*)v;
    return study_thresholds_device(thr->data(), thr->size(), d_thr);
  }
  int frames(const EstChunkDone& c) override {
    const size_t nc = (size_t)pl->n_carrier, K = (size_t)pl->k_atoms, T = (size_t)pl->taps, nb = (size_t)bins.n, p = (size_t)c.p;
    const EstProfilePass ps = est_profile_pass(shape, pl->k_atoms, c.nf);
    // est_delay_kernel's tile holds CH_MAXT picks and TXF_MAX_TAPS channel taps per frame: what rx_plan_create and the generator's
    // checks allow at most, so nothing is left to refuse here
    hipStream_t s = ctx().stream;
    EstProfileSums acc{};
    acc.sums[0] = d_true + p * nc;
    for (int e = 0; e < EST_ROWS; ++e) {
      acc.sums[1 + EST_PROFILE_PER_EST * e + 0] = d_est + (p * EST_ROWS + e) * nc;
      acc.sums[1 + EST_PROFILE_PER_EST * e + 1] = d_err + (p * EST_ROWS + e) * nc;
      acc.sums[1 + EST_PROFILE_PER_EST * e + 2] = d_aerr + (p * EST_ROWS + e) * nc;
    }
    const dim3 ag(ps.acc_grid, ps.acc_quantities);
    if (pl->f64) {
      const EstProfileRows<double> r{{(const c64*)c.h[0], (const c64*)c.h[1], (const c64*)c.h[2], (const c64*)c.h[3]}};
      hipLaunchKernelGGL(est_profile_kernel<double>, ag, dim3(ps.acc_threads), 0, s, c.htrue, c.h_stride, r, c.frame_nmse, c.nf,
                         pl->n_carrier, acc);
    } else {
      const EstProfileRows<float> r{{(const c32*)c.h[0], (const c32*)c.h[1], (const c32*)c.h[2], (const c32*)c.h[3]}};
      hipLaunchKernelGGL(est_profile_kernel<float>, ag, dim3(ps.acc_threads), 0, s, c.htrue, c.h_stride, r, c.frame_nmse, c.nf,
                         pl->n_carrier, acc);
    }
    OFDM_TRY(check_launch("est_profile_kernel"));
    const EstDelayOut dout{d_pick + p * K, d_tamp + p * K, d_npk + p * (T + 1), d_ttamp + p * K, d_outside + p, d_supp + 3 * p,
                           f_picks.sweep ? f_picks.at(T * (size_t)c.at) : nullptr, f_x.sweep ? f_x.at(T * (size_t)c.at) : nullptr};
    hipLaunchKernelGGL(est_delay_kernel, dim3(ps.delay_grid), dim3(ps.delay_threads), 0, s, c.tap_idx, c.tap_x, pl->taps, pl->k_atoms,
                       c.amp, c.amp_stride, dl, c.nf, dout);
    OFDM_TRY(check_launch("est_delay_kernel"));
    const EstHistOut hout{d_hist + p * EST_ROWS * nb, d_below + p * EST_ROWS, d_above + p * EST_ROWS, d_nan + p * EST_ROWS};
    hipLaunchKernelGGL(est_hist_kernel, dim3(ps.hist_grid), dim3(ps.hist_threads), 0, s, c.frame_nmse, (int64_t)EST_ROWS * c.nf,
                       (const double*)d_thr, bins.n, hout);
    return check_launch("est_hist_kernel");
  }
};

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_estimator_profile(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                                      int n_taps, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                      int64_t frames_per_point, int64_t frame0, int mmse_mode, int64_t max_frames_per_chunk,
                                      int hist_bins, double hist_lo_db, double hist_hi_db, uint64_t* errors_out, double* nmse_sums_out,
                                      uint64_t* nmse_dropped_out, uint32_t* frame_errors_out, double* frame_nmse_out,
                                      double* true_amp_sums_out, double* est_amp_sums_out, double* err_sums_out,
                                      double* amp_err_sums_out, uint64_t* nmse_hist_out, uint64_t* nmse_below_out,
                                      uint64_t* nmse_above_out, uint64_t* nmse_nan_out, double* thresholds_out, uint64_t* pick_hist_out,
                                      double* tap_amp_sums_out, uint64_t* n_picks_hist_out, double* true_tap_amp_sums_out,
                                      uint64_t* true_outside_out, uint64_t* support_out, int32_t* picks_out, void* tap_x_out, int flags) {
  const TxfStudyArgs g{h, h_len, tap_delay, tap_power, n_taps, 0, 0, 0, 0.0, nullptr, snr_db, seeds, n_points, frames_per_point, frame0,
                       max_frames_per_chunk, flags};
  EstProfileHook hook;
  hook.pl = pl;
  hook.bins.n = hist_bins; hook.bins.lo = hist_lo_db; hook.bins.hi = hist_hi_db;
  // the table of linear thresholds: made once, on the host; host memory whatever the flags (bins the checks refuse make none)
  std::vector<double> thr;
  if (pl && hest_bins_ok(hook.bins)) {
    thr.resize((size_t)hist_bins + 1);
    hest_thresholds(hook.bins, pl->n_carrier, thr.data());
  }
  hook.thr = &thr;
  hook.out_ = EstProfileOutputs{true_amp_sums_out, est_amp_sums_out, err_sums_out, amp_err_sums_out, nmse_hist_out, nmse_below_out,
                                nmse_above_out, nmse_nan_out, pick_hist_out, tap_amp_sums_out, n_picks_hist_out, true_tap_amp_sums_out,
                                true_outside_out, support_out, picks_out, (c64*)tap_x_out};
  OFDM_TRY(est_study_run(EstStudyCall{pl, g, mmse_mode, errors_out, nmse_sums_out, nmse_dropped_out, frame_errors_out, frame_nmse_out},
                         &hook));
  if (thresholds_out) std::copy(thr.begin(), thr.end(), thresholds_out);
  return OFDM_OK;
}
