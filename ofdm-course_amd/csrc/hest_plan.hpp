// The plan of one call of the channel-estimate capture (ofdm_hest_study.hip): ofdm_rx_hest, the two outputs of estimate_channel
// (T4/estimate_channel.m:6,:8) -- Hest_at_pilots and H_est -- of a batch of the caller's frames behind the receiver's front end and
// fine_sync, with that receiver's scalars, and ofdm_hest_study, the curves of figure 21 of the Task-4 report
// (T4/Main_model_Task_4.m:318-332) summed per carrier and per pilot over the frames of every point of a sweep of the fused
// generator, with the error of the estimate against the frame's true channel.  The argument checks of both entries in the order
// they are made, the chunk the generator's workspace, the receiver's arena and the chunk's rows allow, the launch shape of the
// kernels, and the function every layer shares: the bin of a frame's error on the table of linear thresholds the host makes from
// the dB grid.  Plain C++ with no device or runtime dependency (HEST_HD is empty outside a device compile):
// tests/host/hest_plan_main.cpp runs it under the host sanitizers against tests/hest_cases.py.  The .hip side turns a refusal into
// OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sync_plan.hpp"     // SYNC_LDS_LIMIT; txf_plan.hpp and t4_route.hpp through it

#if defined(__HIPCC__)
#define HEST_HD __host__ __device__
#else
#define HEST_HD
#endif

namespace ofdm {

constexpr int HEST_MAX_BINS = 4096;

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { HEST_REFUSE_FRAMES = TXF_REFUSALS, HEST_REFUSE_BOTH, HEST_REFUSE_TIME_DESYNC, HEST_REFUSE_FREQ_DESYNC, HEST_REFUSE_PILOTS,
       HEST_REFUSE_ROUTE, HEST_REFUSE_BINS, HEST_REFUSE_OUTPUT, HEST_REFUSALS };

// ---- the histogram of the frames' error: n bins of equal width in dB on [lo, hi)
struct HestBins {
  int n = 0;
  double lo = 0.0, hi = 0.0;
};

// ---- the capture of one call
struct HestCapture {
  int time_desync = 1, freq_desync = 1;
  bool study = false;        // ofdm_hest_study: bins is read
  HestBins bins;
  bool out = false;          // an output is given
};

// bins of a histogram in dB: n 1 .. 4096, lo < hi, both finite; the refusal in one wording for every entry that takes them
inline bool hest_bins_ok(const HestBins& b) {
  return b.n >= 1 && b.n <= HEST_MAX_BINS && b.lo < b.hi && b.lo - b.lo == 0.0 && b.hi - b.hi == 0.0;
}

inline int hest_refuse_bins(TxfWhy& w, int id, const char* what, const HestBins& b) {
  return txf_refuse(w, id, "%s: bins must have n 1 .. %d and finite lo < hi (%d, %g, %g)", what, HEST_MAX_BINS, b.n, b.lo, b.hi);
}

// The capture checks, the last of both entries, in this order: time_desync 0 / 1 -> freq_desync 0 / 1 -> at least two pilots (the
// spline of estimate_channel.m:8 needs two knots) -> what else the receiver's route refuses for (time_desync, freq_desync,
// mp_desync 1), in its words -> [the study: bins n 1 .. 4096, lo < hi, both finite] -> an output is given.
inline int hest_check_capture(const TxfShape& s, const HestCapture& c, const char* what, TxfWhy& w) {
  if (!(c.time_desync == 0 || c.time_desync == 1))
    return txf_refuse(w, HEST_REFUSE_TIME_DESYNC, "%s: time_desync must be 0 or 1 (%d)", what, c.time_desync);
  if (!(c.freq_desync == 0 || c.freq_desync == 1))
    return txf_refuse(w, HEST_REFUSE_FREQ_DESYNC, "%s: freq_desync must be 0 or 1 (%d)", what, c.freq_desync);
  if (!(s.np >= 2)) return txf_refuse(w, HEST_REFUSE_PILOTS, "%s: estimate_channel needs at least two pilot carriers (%d)", what, s.np);
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, c.time_desync, c.freq_desync, 1, 0};
  T4Route r;
  const char* why = nullptr;
  if (t4_route_choose(t4, r, &why) != T4_ROUTE_OK) return txf_refuse(w, HEST_REFUSE_ROUTE, "%s: %s", what, why);
  if (c.study && !hest_bins_ok(c.bins)) return hest_refuse_bins(w, HEST_REFUSE_BINS, what, c.bins);
  if (!c.out) return txf_refuse(w, HEST_REFUSE_OUTPUT, "%s: no output is given", what);
  return TXF_OK;
}

// ---- ofdm_rx_hest.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, rx) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in band,
//   Nfft / T_guard) -> n_frames 0 .. 2^31 - 1 -> the capture (above)
inline int hest_rx_prelude(const TxfShape* plan, bool rx, bool f64_flag, int64_t n_frames, const HestCapture& cap, TxfWhy& w) {
  static const char* const WHAT = "rx_hest";
  if (const int id = txf_check_args(plan && rx, WHAT, w)) return id;
  if (const int id = txf_check_plan(*plan, f64_flag, 0, 0, WHAT, w)) return id;
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, HEST_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  return hest_check_capture(*plan, cap, WHAT, w);
}

// ---- ofdm_hest_study.  The order of its checks: the front every study shares (txf_study_prelude: the generator's arguments,
// max_frames_per_chunk 0 .. 65535, the receiver's limit) -> the capture (above)
inline int hest_study_prelude(const TxfCall& c, bool both_channels, const HestCapture& cap, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "hest_study";
  if (const int id = txf_study_prelude(c, both_channels, HEST_REFUSE_BOTH, WHAT, ch, g, w, 65535)) return id;
  return hest_check_capture(*c.plan, cap, WHAT, w);
}

// ---- the chunk of the study: frames of one point, budgeted as the Task-4 sweep budgets its chunks (the generator's regions with
// the RX region and the receiver's arena, on twice the workspace budget) and, beside them, per frame
//   per carrier  4 doubles (|H_est|, |H|, |H - H_est|^2, (|H_est| - |H|)^2) and 1 byte (H_est not finite)      33 N_carrier
//   per pilot    2 doubles (|Hest_at_pilots|, |H - Hest_at_pilots|^2) and 1 byte (not finite)                   17 Np
//   scalars      the two error sums, TgPosition, FreqOffset (8 bytes each), IFO, status (4 each)                40
constexpr size_t HEST_CARRIER_ROWS = 4, HEST_PILOT_ROWS = 2;
constexpr size_t HEST_SCALAR_BYTES = 40;

inline size_t hest_row_bytes(const TxfShape& s) {
  return (HEST_CARRIER_ROWS * sizeof(double) + 1) * (size_t)s.n_carrier + (HEST_PILOT_ROWS * sizeof(double) + 1) * (size_t)s.np +
         HEST_SCALAR_BYTES;
}

inline int64_t hest_chunk(const TxfShape& s, const TxfUse& u, int64_t frames_per_point, int64_t user_cap, size_t budget = 2 * TXF_WS_BUDGET) {
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, 0, 0, 0, 0};
  return txf_chunk(s, u, frames_per_point, user_cap, budget, t4_frame_bytes(t4, s.frame_words) + hest_row_bytes(s));
}

// ---- the launch shape.  hest_capture_kernel: workgroups of HEST_THREADS threads cover whole frames, the carriers across the
// lanes: from 256 carriers on one frame per workgroup (a lane walks the carriers with a stride of 256), below that a frame takes
// the next power of two of lanes (at least 16) and a workgroup holds 256 / lanes frames, so that no wavefront is launched part
// empty.  Static LDS: the taps of every frame of the workgroup.  hest_frame_sum_kernel: one workgroup of 256 threads per frame, the
// four wave partials.  hest_accumulate_kernel: the studies' accumulate shape (txf_plan.hpp: STUDY_ACC_*) over the carriers (pilots)
// of one quantity each, no tail workgroup; its tile holds the doubles and the bytes beside them, 9 bytes per entry.
constexpr int HEST_THREADS = 256;
constexpr int HEST_MIN_LANES = 16;
constexpr int HEST_MAX_FRAMES_PER_WG = HEST_THREADS / HEST_MIN_LANES;
constexpr size_t HEST_CAPTURE_LDS = 16 * (size_t)HEST_MAX_FRAMES_PER_WG * TXF_MAX_TAPS;
constexpr size_t HEST_ACC_LDS = (sizeof(double) + 1) * STUDY_ACC_TILE * STUDY_ACC_COLS;

constexpr int hest_lanes(int n_carrier) {
  int l = HEST_MIN_LANES;
  while (l < HEST_THREADS && l < n_carrier) l *= 2;
  return l;
}

static_assert(HEST_CAPTURE_LDS == 16384 && HEST_CAPTURE_LDS <= SYNC_LDS_LIMIT, "the capture kernel's LDS");
static_assert(HEST_ACC_LDS == 36864 && HEST_ACC_LDS <= SYNC_LDS_LIMIT, "the accumulating kernel's LDS");
static_assert(hest_lanes(1) == 16 && hest_lanes(64) == 64 && hest_lanes(65) == 128 && hest_lanes(256) == 256 && hest_lanes(4096) == 256,
              "the lanes of a frame");

struct HestPass {
  int threads;               // HEST_THREADS
  int lanes;                 // of a frame: hest_lanes(N_carrier)
  int frames_per_wg;         // threads / lanes
  size_t lds;                // static LDS of the capture kernel
  unsigned grid;             // ceil(frames / frames_per_wg)
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // ceil(N_carrier / STUDY_ACC_COLS), times HEST_CARRIER_ROWS quantities in y
  unsigned acc_grid_pilots;  // ceil(Np / STUDY_ACC_COLS), times HEST_PILOT_ROWS quantities in y
  size_t acc_lds;            // static LDS of the accumulating kernel
};

inline HestPass hest_pass(const TxfShape& s, int64_t frames) {
  HestPass p{};
  p.threads = HEST_THREADS;
  p.lanes = hest_lanes(s.n_carrier);
  p.frames_per_wg = HEST_THREADS / p.lanes;
  p.lds = HEST_CAPTURE_LDS;
  p.grid = (unsigned)((frames + p.frames_per_wg - 1) / p.frames_per_wg);
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(s.n_carrier, 0);
  p.acc_grid_pilots = study_acc_grid(s.np, 0);
  p.acc_lds = HEST_ACC_LDS;
  return p;
}

// ---- the histogram of the frames by 10 log10(frame_nmse / N_carrier) on the dB grid.  The device never takes a logarithm: the
// host turns the n + 1 edges lo + i (hi - lo) / n (the last one hi itself) into linear thresholds N_carrier 10^(edge / 10) once, in
// double; the table is an argument of the call and an output of it, and every layer finds the bin by comparisons against it.
inline void hest_thresholds(const HestBins& b, int n_carrier, double* thr) {
  for (int i = 0; i <= b.n; ++i) {
    const double edge = i == b.n ? b.hi : b.lo + (b.hi - b.lo) * (double)i / (double)b.n;
    thr[i] = (double)n_carrier * std::pow(10.0, edge / 10.0);
  }
}

enum { HEST_BIN_BELOW = -1, HEST_BIN_ABOVE = -2, HEST_BIN_NAN = -3 };

// The bin of v on thr[0 .. n] (not decreasing): HEST_BIN_NAN for a NaN, HEST_BIN_BELOW for v < thr[0], HEST_BIN_ABOVE for
// v >= thr[n] (+inf too), else the last b with thr[b] <= v, by bisection.  Comparisons only: every layer gets the same bin.
HEST_HD inline int hest_bin(double v, const double* thr, int n) {
  if (v != v) return HEST_BIN_NAN;
  if (v < thr[0]) return HEST_BIN_BELOW;
  if (!(v < thr[n])) return HEST_BIN_ABOVE;
  int lo = 0, hi = n;                                 // thr[lo] <= v < thr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) / 2;
    if (v < thr[mid]) hi = mid;
    else lo = mid;
  }
  return lo;
}

}  // namespace ofdm
