// The plan of one call of the estimator profile (ofdm_est_profile.hip): ofdm_estimator_profile, the two pictures the Task-5 drivers
// draw beside their error numbers -- |H_freq| against |H_est_LS|, |H_est_MMSE|, |H_est_MP|, |H_est_OMP| over the carriers
// (T5/Main_model_Task_5.m:207-231) and |H_tau| against the picked delays of OMP_estimate (:238-242) -- summed over the frames of
// every point of the estimator study's sweep, with the histogram of the frames' error.  The call is the estimator study's
// (est_plan.hpp) with more outputs: the same checks under its own name, then the bins of the histogram as the channel study
// takes them (hest_plan.hpp), the same chunk, and the launch shapes of the three kernels it adds.  Plain C++ with no device or
// runtime dependency: tests/host/est_profile_plan_main.cpp runs it under the host sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

#include "chain_route.hpp"   // CH_MAXT
#include "est_plan.hpp"
#include "hest_plan.hpp"

namespace ofdm {

// the refusals of the entry: those of the estimator study, or its own
enum { EST_PROFILE_REFUSE_BINS = EST_REFUSALS, EST_PROFILE_REFUSALS };

// The order of the checks: everything est_study_prelude refuses up to and including mmse_mode, in its words under the name
// estimator_profile -> bins n 1 .. 4096, lo < hi, both finite (the channel study's wording) -> an output is given.
inline int est_profile_prelude(const TxfCall& c, bool both_channels, const EstWanted& e, const HestBins& bins, TxfChannel& ch,
                               TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "estimator_profile";
  EstWanted front = e;
  front.out = true;                                   // the output check comes last, behind the bins
  if (const int id = est_study_prelude(c, both_channels, front, ch, g, w, WHAT)) return id;
  if (!hest_bins_ok(bins)) return hest_refuse_bins(w, EST_PROFILE_REFUSE_BINS, WHAT, bins);
  if (!e.out) return txf_refuse(w, EST_REFUSE_OUTPUT, "%s: no output is given", WHAT);
  return TXF_OK;
}

// ---- the chunk.  The profile keeps no rows of its own: the per-carrier kernel reads the body's four H buffers, the truth and the
// chunk's frame_nmse, the delay kernel the plan's tap workspace and the frames' amplitudes -- all of them in est_plan.hpp's budget
// already -- and with want_frames the picks and coefficients go to the caller's arrays over the whole sweep.  So the bytes it adds
// per frame are none, and its chunk is the study's.
inline size_t est_profile_row_bytes(const TxfShape&, int /*taps*/) { return 0; }

inline int64_t est_profile_chunk(const TxfShape& s, const TxfUse& u, int taps, int64_t frames_per_point, int64_t user_cap,
                                 size_t budget = 2 * TXF_WS_BUDGET) {
  return txf_chunk(s, u, frames_per_point, user_cap, budget,
                   est_body_frame_bytes(s) + est_row_bytes(s, taps) + est_profile_row_bytes(s, taps));
}

// ---- the launch shapes.
// est_profile_kernel: the studies' accumulate shape (txf_plan.hpp: STUDY_ACC_*) over the carriers, one quantity per blockIdx.y:
//   quantity 0 the truth's amplitude, then for each estimator its amplitude, its squared error and its squared amplitude error.
// est_delay_kernel: workgroups of EST_DELAY_THREADS threads, one thread per delay of the dictionary; the chunk's picks, the amplitude
//   of their coefficients and of the channel's taps staged EST_DELAY_FRAMES frames at a time in LDS.
// est_hist_kernel: one thread per frame and estimator.
constexpr int EST_PROFILE_PER_EST = 3;                // est_amp, err, amp_err
constexpr int EST_PROFILE_QUANTITIES = 1 + EST_PROFILE_PER_EST * EST_ROWS;
constexpr int EST_DELAY_THREADS = 256;
constexpr int EST_DELAY_FRAMES = 32;
constexpr size_t EST_DELAY_LDS =
    (size_t)EST_DELAY_FRAMES * ((sizeof(int32_t) + sizeof(double)) * (size_t)CH_MAXT + sizeof(double) * (size_t)TXF_MAX_TAPS);
constexpr int EST_HIST_THREADS = 256;

static_assert(EST_PROFILE_QUANTITIES == 13, "the quantities of the per-carrier kernel");
static_assert(EST_DELAY_LDS == 28672 && EST_DELAY_LDS <= SYNC_LDS_LIMIT, "the delay kernel's LDS");
static_assert(EST_DELAY_FRAMES <= EST_DELAY_THREADS, "one thread per frame of the tile");

struct EstProfilePass {
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // ceil(N_carrier / STUDY_ACC_COLS), times EST_PROFILE_QUANTITIES in y
  unsigned acc_quantities;
  size_t acc_lds;            // STUDY_ACC_LDS
  int delay_threads;         // EST_DELAY_THREADS
  unsigned delay_grid;       // ceil(K / EST_DELAY_THREADS)
  size_t delay_lds;
  int hist_threads;          // EST_HIST_THREADS
  unsigned hist_grid;        // ceil(4 frames / EST_HIST_THREADS)
};

inline EstProfilePass est_profile_pass(const TxfShape& s, int k_atoms, int64_t frames) {
  EstProfilePass p{};
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(s.n_carrier, 0);
  p.acc_quantities = EST_PROFILE_QUANTITIES;
  p.acc_lds = STUDY_ACC_LDS;
  p.delay_threads = EST_DELAY_THREADS;
  p.delay_grid = (unsigned)((k_atoms + EST_DELAY_THREADS - 1) / EST_DELAY_THREADS);
  p.delay_lds = EST_DELAY_LDS;
  p.hist_threads = EST_HIST_THREADS;
  p.hist_grid = (unsigned)((EST_ROWS * frames + EST_HIST_THREADS - 1) / EST_HIST_THREADS);
  return p;
}

}  // namespace ofdm
