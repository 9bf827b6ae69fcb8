// The plan of one call of the coarse-sync capture (ofdm_sync_study.hip): ofdm_rx_acf, abs(AutoCorr) of AutoCorrFunction(frame,
// WidthWindow, Nfft) for a batch of the caller's frames with TgPosition, FreqOffset and the catch-branch flag of each
// (T4/AutoCorrFunction.m:3-27, plotted at T4/Main_model_Task_4.m:282-287), and ofdm_sync_study, those curves summed over the frames
// of every point of a sweep of the fused generator with the histograms of TgPosition and the fractional frequency-offset error
// (T4/Main_model_Task_4.m:113-135).  The argument checks of both entries in the order they are made, the chunk the generator's
// workspace and the chunk's rows allow, the launch shape of the two kernels, and the two small functions every layer shares: the
// guard-phase bin of a frame and its wrapped fractional error.  Plain C++ with no device or runtime dependency (SYNC_HD is empty
// outside a device compile): tests/host/sync_plan_main.cpp runs it under the host sanitizers against tests/sync_cases.py.  The .hip
// side turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
//
// The integer frequency offset is out of scope: remove_IFO needs the derotated stream and a transform, and the Task-4 sweep's
// cfo_abs_err already covers FreqOffset + IFO - Freq_Shift.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "txf_plan.hpp"      // TxfShape, TxfUse, TxfCall, txf_check_plan, txf_study_prelude, txf_chunk

#if defined(__HIPCC__)
#define SYNC_HD __host__ __device__
#else
#define SYNC_HD
#endif

namespace ofdm {

// sync_core.hpp's ACF_TILE / ACF_THREADS / ACF_MAXW and the bytes of an acf4<T> and a cx<T>, restated (ofdm_sync_study.hip asserts them)
constexpr int SYNC_ACF_TILE = 1024;
constexpr int SYNC_ACF_THREADS = 256;
constexpr int SYNC_ACF_MAXW = 1024;

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { SYNC_REFUSE_FRAMES = TXF_REFUSALS, SYNC_REFUSE_BOTH, SYNC_REFUSE_WIDTH, SYNC_REFUSE_SHORT, SYNC_REFUSE_OUTPUT, SYNC_REFUSALS };

// ---- the capture: the curve of one frame has n_out = frame_samples - WidthWindow - Nfft lags (AutoCorrFunction.m:3)
struct SyncCapture {
  int64_t width = 0;         // WidthWindow
  bool out = false;          // an output is given (ofdm_rx_acf: any of its five; the study: acf_sums_out)
};

inline int64_t sync_n_out(const TxfShape& s, int64_t width) {
  return ((int64_t)s.nfft + s.t_guard) * s.n_symb - width - s.nfft;
}

// The capture checks, the last of both entries, in this order: WidthWindow 1 .. SYNC_ACF_MAXW -> n_out >= 1 -> an output is given.
inline int sync_check_capture(const TxfShape& s, const SyncCapture& c, const char* what, TxfWhy& w) {
  if (!(c.width >= 1 && c.width <= SYNC_ACF_MAXW))
    return txf_refuse(w, SYNC_REFUSE_WIDTH, "%s: WidthWindow must be 1 .. %d (%lld)", what, SYNC_ACF_MAXW, (long long)c.width);
  if (!(sync_n_out(s, c.width) >= 1))
    return txf_refuse(w, SYNC_REFUSE_SHORT, "%s: a frame of %lld samples is shorter than WidthWindow + Nfft + 1 (%lld + %d + 1)", what,
                      (long long)(((int64_t)s.nfft + s.t_guard) * s.n_symb), (long long)c.width, s.nfft);
  if (!c.out) return txf_refuse(w, SYNC_REFUSE_OUTPUT, "%s: no output is given", what);
  return TXF_OK;
}

// ---- ofdm_rx_acf.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, rx) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in band,
//   Nfft / T_guard) -> n_frames 0 .. 2^31 - 1 -> the capture (above)
inline int sync_rx_prelude(const TxfShape* plan, bool rx, bool f64_flag, int64_t n_frames, const SyncCapture& cap, TxfWhy& w) {
  static const char* const WHAT = "rx_acf";
  if (const int id = txf_check_args(plan && rx, WHAT, w)) return id;
  if (const int id = txf_check_plan(*plan, f64_flag, 0, 0, WHAT, w)) return id;
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, SYNC_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  return sync_check_capture(*plan, cap, WHAT, w);
}

// ---- ofdm_sync_study.  The order of its checks: the front every study shares (txf_study_prelude: the generator's arguments,
// max_frames_per_chunk >= 0) -> the capture (above)
inline int sync_study_prelude(const TxfCall& c, bool both_channels, const SyncCapture& cap, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "sync_study";
  if (const int id = txf_study_prelude(c, both_channels, SYNC_REFUSE_BOTH, WHAT, ch, g, w)) return id;
  return sync_check_capture(*c.plan, cap, WHAT, w);
}

// ---- the chunk of the study: frames of one point, budgeted on the generator's regions with the RX region (txf_study_use) and,
// beside the workspace, per frame one row of n_out doubles (|rho| of every lag) and the frame's scalars (TgPosition, FreqOffset,
// the wrapped error: 8 bytes each; the status: 4, padded to 8).  The peak wants no second row: it folds the rows the sum reads.
inline TxfUse sync_use(bool scr, bool imp, int fade_taps) { return txf_study_use(scr, imp, fade_taps); }   // the name callers know

constexpr size_t SYNC_SCALAR_BYTES = 32;

inline size_t sync_row_bytes(const TxfShape& s, int64_t width) { return sizeof(double) * (size_t)sync_n_out(s, width) + SYNC_SCALAR_BYTES; }

inline int64_t sync_chunk(const TxfShape& s, const TxfUse& u, int64_t frames_per_point, int64_t user_cap, int64_t width,
                          size_t budget = TXF_WS_BUDGET) {
  return txf_chunk(s, u, frames_per_point, user_cap, budget, sync_row_bytes(s, width));
}

// ---- the launch shape.  sync_capture_kernel: one workgroup of SYNC_ACF_THREADS threads per frame; its dynamic LDS is the prefix
// table of acf_tile, SYNC_ACF_TILE + WidthWindow + 1 entries of four sums in the plan's precision, and behind it one tile of rho.
// sync_accumulate_kernel: the studies' accumulate launch (txf_plan.hpp: STUDY_ACC_*) over the n_out lags, with the tail workgroup for
// the chunk's wrapped errors.
constexpr size_t sync_table_bytes(bool f64, int width) { return (f64 ? 32 : 16) * (size_t)(SYNC_ACF_TILE + width + 1); }
constexpr size_t sync_capture_lds(bool f64, int width) { return sync_table_bytes(f64, width) + (f64 ? 16 : 8) * (size_t)SYNC_ACF_TILE; }

// The largest case, double at WidthWindow 1024, is 81 952 bytes: inside the limit, one workgroup per CU (two would need 163 904 of
// the 163 840 bytes of a CU).  Float at 1024: 40 976, three per CU; the Task-4 width of 128: 53 280 and 26 640, three and six.
static_assert(sync_capture_lds(true, SYNC_ACF_MAXW) == 81952 && sync_capture_lds(true, SYNC_ACF_MAXW) <= SYNC_LDS_LIMIT,
              "the capture kernel's LDS at its largest");

struct SyncPass {
  int threads;               // SYNC_ACF_THREADS
  unsigned grid;             // frames: one workgroup each (a chunk holds at most 65535)
  size_t lds;                // dynamic LDS of the capture kernel
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // ceil(n_out / STUDY_ACC_COLS) + 1
};

inline SyncPass sync_pass(const TxfShape& s, int64_t width, int64_t frames) {
  SyncPass p{};
  p.threads = SYNC_ACF_THREADS;
  p.grid = (unsigned)frames;
  p.lds = sync_capture_lds(s.f64 != 0, (int)width);
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(sync_n_out(s, width), 1);
  return p;
}

// ---- the two functions of a frame's scalars, one definition for the device code, the stand-alone program and (through it) the
// Python twins of tests/sync_cases.py.
// The guard-phase bin: (TgPosition - 1 + sto) mod (Nfft + T_guard), in 0 .. Nfft + T_guard - 1 for either sign of sto (the frame's
// Time_Delay, add_STO's nSTO).  A delay moves every guard interval by -sto, so the bin of a frame does not depend on its draw.
SYNC_HD inline int64_t sync_phase_bin(int64_t tg_position, int64_t sto, int64_t stride) {
  const int64_t a = (tg_position - 1) % stride, b = sto % stride;      // each in -(stride - 1) .. stride - 1: the sum fits for any stride <= 2^62
  const int64_t r = (a + b) % stride;
  return r < 0 ? r + stride : r;
}

// The wrapped fractional error of FreqOffset against the frame's Freq_Shift: ffo_true = cfo - rint(cfo), d = FreqOffset - ffo_true,
// e = d - rint(d), in double with ties to even.  NaN for a NaN FreqOffset.
SYNC_HD inline double sync_ffo_err(double freq_offset, double cfo) {
  const double ffo_true = cfo - ::rint(cfo);
  const double d = freq_offset - ffo_true;
  return d - ::rint(d);
}

}  // namespace ofdm
