// The plan of one call of the received-spectrum capture (ofdm_spectrum.hip): ofdm_rx_spectrum, |fft| of windows of the caller's
// frames (abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard))), T3/Main_model_Task_3.m:138, T5/Main_model_Task_5.m:131), and
// ofdm_spectrum_study, the power per bin summed over the frames of every point of a sweep of the fused generator.  The argument
// checks of both entries in the order they are made, the chunk the generator's workspace and the chunk's power rows allow, and the
// launch shape of the two kernels -- decided before anything is launched or allocated.  Plain C++ with no device or runtime
// dependency: tests/host/spectrum_plan_main.cpp runs it under the host sanitizers against tests/spectrum_cases.py.  The .hip side
// turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "txf_plan.hpp"      // TxfShape, TxfUse, TxfCall, txf_check_plan, txf_study_prelude, txf_chunk

namespace ofdm {

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { SPEC_REFUSE_FRAMES = TXF_REFUSALS, SPEC_REFUSE_BOTH, SPEC_REFUSE_FIRST, SPEC_REFUSE_WINDOWS, SPEC_REFUSE_END,
       SPEC_REFUSE_OUTPUT, SPEC_REFUSALS };

// ---- the capture: window w = 0 .. n_windows - 1 of a frame is its samples first + w (Nfft + T_guard) .. + Nfft - 1 (0-based)
struct SpecCapture {
  int64_t first = 0, n_windows = 0;
  bool out = false;          // an output is given (ofdm_rx_spectrum: amp_out or power_out; the study: power_sums_out)
};

// The capture checks, the last of both entries, in this order: first >= 0 -> n_windows >= 1 -> the last window ends at or before
// frame_samples -> an output is given.  The end is compared without forming first + (n_windows - 1) * (Nfft + T_guard) + Nfft,
// which may not fit 64 bits: the room behind the first window is counted in whole strides.
inline int spectrum_check_capture(const TxfShape& s, const SpecCapture& c, const char* what, TxfWhy& w) {
  const int64_t stride = (int64_t)s.nfft + s.t_guard, frame_samples = stride * s.n_symb;
  if (!(c.first >= 0)) return txf_refuse(w, SPEC_REFUSE_FIRST, "%s: first must be >= 0 (%lld)", what, (long long)c.first);
  if (!(c.n_windows >= 1)) return txf_refuse(w, SPEC_REFUSE_WINDOWS, "%s: n_windows must be >= 1 (%lld)", what, (long long)c.n_windows);
  const int64_t room = frame_samples - s.nfft;       // the last start that fits
  if (!(room >= 0 && c.first <= room && c.n_windows - 1 <= (room - c.first) / stride))
    return txf_refuse(w, SPEC_REFUSE_END, "%s: %lld windows from sample %lld on end behind the frame of %lld samples", what,
                      (long long)c.n_windows, (long long)c.first, (long long)frame_samples);
  if (!c.out) return txf_refuse(w, SPEC_REFUSE_OUTPUT, "%s: no output is given", what);
  return TXF_OK;
}

// ---- ofdm_rx_spectrum.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, rx) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in band,
//   Nfft / T_guard) -> n_frames 0 .. 2^31 - 1 -> the capture (above)
inline int spectrum_rx_prelude(const TxfShape* plan, bool rx, bool f64_flag, int64_t n_frames, const SpecCapture& cap, TxfWhy& w) {
  static const char* const WHAT = "rx_spectrum";
  if (const int id = txf_check_args(plan && rx, WHAT, w)) return id;
  if (const int id = txf_check_plan(*plan, f64_flag, 0, 0, WHAT, w)) return id;
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, SPEC_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  return spectrum_check_capture(*plan, cap, WHAT, w);
}

// ---- ofdm_spectrum_study.  The order of its checks: the front every study shares (txf_study_prelude: the generator's arguments,
// max_frames_per_chunk >= 0) -> the capture (above)
inline int spectrum_study_prelude(const TxfCall& c, bool both_channels, const SpecCapture& cap, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "spectrum_study";
  if (const int id = txf_study_prelude(c, both_channels, SPEC_REFUSE_BOTH, WHAT, ch, g, w)) return id;
  return spectrum_check_capture(*c.plan, cap, WHAT, w);
}

// ---- the chunk of the study: frames of one point, budgeted on the generator's regions with the RX region (txf_study_use) and,
// beside the workspace, the chunk's power rows (Nfft doubles per frame; with the peak wanted a second row per frame, the maximum
// over the frame's windows)
inline TxfUse spectrum_use(bool scr, bool imp, int fade_taps) { return txf_study_use(scr, imp, fade_taps); }   // the name callers know

inline size_t spectrum_row_bytes(const TxfShape& s, bool peak) { return sizeof(double) * (size_t)s.nfft * (peak ? 2 : 1); }

inline int64_t spectrum_chunk(const TxfShape& s, const TxfUse& u, int64_t frames_per_point, int64_t user_cap, bool peak,
                              size_t budget = TXF_WS_BUDGET) {
  return txf_chunk(s, u, frames_per_point, user_cap, budget, spectrum_row_bytes(s, peak));
}

// ---- the launch shape.  spectrum_kernel: a transform of Nfft / 8 threads per frame, every window of the frame in turn;
// workgroups of at least 256 threads hold 256 / (Nfft / 8) frames (fft_core.hpp's rule, restated; ofdm_spectrum.hip asserts it).
// spectrum_accumulate_kernel: the studies' accumulate launch (txf_plan.hpp: STUDY_ACC_*) over the Nfft bins, no tail workgroup.
struct SpecPass {
  int threads;               // per workgroup: max(256, Nfft / 8)
  int frames_per_wg;         // threads / (Nfft / 8)
  size_t lds;                // static LDS: frames_per_wg transforms of Nfft + Nfft / 8 + 8 padded elements
  unsigned grid;             // ceil(frames / frames_per_wg)
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // Nfft / STUDY_ACC_COLS
};

inline SpecPass spectrum_pass(const TxfShape& s, int64_t frames) {
  SpecPass p{};
  p.threads = std::max(256, s.nfft / 8);
  p.frames_per_wg = p.threads / (s.nfft / 8);
  p.lds = (size_t)(s.f64 ? 16 : 8) * p.frames_per_wg * (size_t)(s.nfft + s.nfft / 8 + 8);
  p.grid = (unsigned)((frames + p.frames_per_wg - 1) / p.frames_per_wg);
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(s.nfft, 0);
  return p;
}

}  // namespace ofdm
