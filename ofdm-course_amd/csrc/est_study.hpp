// The call of the estimator study (ofdm_est_study.hip) as its two entries share it: ofdm_estimator_study, and
// ofdm_estimator_profile (ofdm_est_profile.hip), which is the same call with more outputs.  est_study_run makes the checks, stages
// the study's tables, generates every chunk (txf_sweep_points), runs the truth, the estimator body and the study's three kernels on
// it; an entry with outputs of its own hooks into the places where the study stages and where a chunk is done.
#pragma once

#include "est_body.hpp"
#include "est_plan.hpp"
#include "txf_study.hpp"

namespace ofdm {

struct EstStudyCall {
  ofdm_rx_plan* pl;
  TxfStudyArgs g;                // sto / cfo off, no register
  int mmse_mode;
  uint64_t* errors_out;
  double* nmse_sums_out;
  uint64_t* nmse_dropped_out;
  uint32_t* frame_errors_out;
  double* frame_nmse_out;
};

// what a chunk leaves behind once the study's kernels have run on it, all in device memory
struct EstChunkDone {
  int64_t nf, p, at;             // frames of the chunk, its point, the sweep index of its first frame
  const void* h[EST_ROWS];       // [nf][N_carrier] in the plan's precision: LS, MMSE, MP, OMP
  const int32_t* tap_idx;        // [nf][taps] OMP's picks, 0-based, -1 = not made
  const c64* tap_x;              // [nf][taps]
  const c64* htrue;              // the true H, row f at f * h_stride (0: a static channel, one row)
  int64_t h_stride;
  const double* frame_nmse;      // [nf][4]
  const c64* amp;                // the taps' amplitudes, frame f at f * amp_stride (0: the static channel's)
  int64_t amp_stride;
};

struct EstStudyHook {
  virtual ~EstStudyHook() = default;
  // the checks of the entry in front of the body's: est_study_prelude, or the entry's own around it
  virtual int prelude(const TxfCall& c, bool both_channels, const EstWanted& e, TxfChannel& ch, TxfGains& g, TxfWhy& w) = 0;
  virtual const char* what() const = 0;                       // the entry as the front's refusals name it
  virtual bool out() const = 0;                               // an output of its own is given
  virtual int64_t chunk(const TxfShape& s, const TxfUse& u, int taps, int64_t frames_per_point, int64_t user_cap) = 0;
  virtual int tables(Stage& st, size_t n_points, size_t frames_per_point) = 0;   // its outputs, beside the study's, zeroed
  virtual int begin(Stage& st, const TxfDelays& dl, int64_t CH) = 0;             // its scratch, once the chunk is known
  virtual int frames(const EstChunkDone& c) = 0;                                 // a chunk is done
};

int est_study_run(const EstStudyCall& call, EstStudyHook* hook);

}  // namespace ofdm
