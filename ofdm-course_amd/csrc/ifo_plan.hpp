// The plan of one call of the integer-CFO capture (ofdm_ifo_study.hip): ofdm_rx_ifo, the spectrum remove_IFO thresholds --
// abs(fft(rx_signal(Nfft+1 : 2*Nfft))), T4/remove_IFO.m:5 -- of a batch of the caller's frames with IFO = inds(1) - 1 (:6-8), the
// number of bins above 0.77 and the scalars of the AutoCorrFunction stage in front, and ofdm_ifo_study, those rows summed over the
// frames of every point of a sweep of the fused generator with the histograms of IFO and of its error against the frame's own
// Freq_Shift (T4/Main_model_Task_4.m:113-135, figure 13b of the Task-4 report).  Two call sites of remove_IFO can be looked at:
// stage 0, the received frame as it is (T4:124-125), and stage 1, the stream the receiver hands it (T4:278-303: the two add_STO with
// time_desync, add_CFO(-FreqOffset)).  The argument checks of both entries in the order they are made, the chunk the generator's
// workspace and the chunk's rows allow, the launch shape of the two kernels, and the two small functions every layer shares: the
// bin of IFO - rint(Freq_Shift) and the total frequency error.  Plain C++ with no device or runtime dependency (IFO_HD is empty
// outside a device compile): tests/host/ifo_plan_main.cpp runs it under the host sanitizers against tests/ifo_cases.py.  The .hip
// side turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sync_plan.hpp"     // SYNC_LDS_LIMIT; txf_plan.hpp and t4_route.hpp through it

#if defined(__HIPCC__)
#define IFO_HD __host__ __device__
#else
#define IFO_HD
#endif

namespace ofdm {

enum { IFO_STAGE_RAW = 0, IFO_STAGE_RECEIVER = 1 };
constexpr int64_t IFO_MAX_SPAN = 4096;

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { IFO_REFUSE_FRAMES = TXF_REFUSALS, IFO_REFUSE_BOTH, IFO_REFUSE_STAGE, IFO_REFUSE_TIME_DESYNC, IFO_REFUSE_SHORT, IFO_REFUSE_ROUTE,
       IFO_REFUSE_SPAN, IFO_REFUSE_OUTPUT, IFO_REFUSALS };

// ---- the capture of one call
struct IfoCapture {
  int stage = IFO_STAGE_RECEIVER;
  int time_desync = 1;
  bool study = false;        // ofdm_ifo_study: err_span is read
  int64_t err_span = 0;
  bool out = false;          // an output is given
};

// The capture checks, the last of both entries, in this order: stage 0 / 1 -> time_desync 0 / 1 -> the frame holds
// rx_signal(Nfft+1 : 2*Nfft) (in the words of t4_route.hpp) -> what else the receiver's route refuses for (time_desync, freq_desync
// 1), in its words: the AutoCorrFunction stage in front is the receiver's (T_guard 1 .. 1024, two pilots) -> [the study: err_span
// 1 .. 4096] -> an output is given.
inline int ifo_check_capture(const TxfShape& s, const IfoCapture& c, const char* what, TxfWhy& w) {
  if (!(c.stage == IFO_STAGE_RAW || c.stage == IFO_STAGE_RECEIVER))
    return txf_refuse(w, IFO_REFUSE_STAGE, "%s: stage must be 0 (the received frame) or 1 (the receiver's stream) (%d)", what, c.stage);
  if (!(c.time_desync == 0 || c.time_desync == 1))
    return txf_refuse(w, IFO_REFUSE_TIME_DESYNC, "%s: time_desync must be 0 or 1 (%d)", what, c.time_desync);
  if (((int64_t)s.nfft + s.t_guard) * s.n_symb < 2 * (int64_t)s.nfft)
    return txf_refuse(w, IFO_REFUSE_SHORT, "%s: rx_signal(Nfft+1:2*Nfft) exceeds the frame", what);
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, c.time_desync, 1, 0, 0};
  T4Route r;
  const char* why = nullptr;
  if (t4_route_choose(t4, r, &why) != T4_ROUTE_OK) return txf_refuse(w, IFO_REFUSE_ROUTE, "%s: %s", what, why);
  if (c.study && !(c.err_span >= 1 && c.err_span <= IFO_MAX_SPAN))
    return txf_refuse(w, IFO_REFUSE_SPAN, "%s: err_span must be 1 .. %lld (%lld)", what, (long long)IFO_MAX_SPAN, (long long)c.err_span);
  if (!c.out) return txf_refuse(w, IFO_REFUSE_OUTPUT, "%s: no output is given", what);
  return TXF_OK;
}

// ---- ofdm_rx_ifo.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, rx) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in band,
//   Nfft / T_guard) -> n_frames 0 .. 2^31 - 1 -> the capture (above)
inline int ifo_rx_prelude(const TxfShape* plan, bool rx, bool f64_flag, int64_t n_frames, const IfoCapture& cap, TxfWhy& w) {
  static const char* const WHAT = "rx_ifo";
  if (const int id = txf_check_args(plan && rx, WHAT, w)) return id;
  if (const int id = txf_check_plan(*plan, f64_flag, 0, 0, WHAT, w)) return id;
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, IFO_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  return ifo_check_capture(*plan, cap, WHAT, w);
}

// ---- ofdm_ifo_study.  The order of its checks: the front every study shares (txf_study_prelude: the generator's arguments,
// max_frames_per_chunk >= 0) -> the capture (above)
inline int ifo_study_prelude(const TxfCall& c, bool both_channels, const IfoCapture& cap, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "ifo_study";
  if (const int id = txf_study_prelude(c, both_channels, IFO_REFUSE_BOTH, WHAT, ch, g, w)) return id;
  return ifo_check_capture(*c.plan, cap, WHAT, w);
}

// ---- the chunk of the study: frames of one point, budgeted on the generator's regions with the RX region (txf_study_use) and,
// beside the workspace, per frame one row of Nfft doubles (|S| of every bin), Nfft bytes (the bins above the threshold) and the
// frame's scalars (TgPosition, FreqOffset, the total error: 8 bytes each; IFO, status, the count of bins above: 4 each, padded to
// 40).  The AutoCorrFunction stage in front keeps nothing per frame on its search route (with OFDM_T4_FULL_ACF, an A/B switch, the
// curve lives in the receiver's arena and is not budgeted here).
constexpr size_t IFO_SCALAR_BYTES = 40;

inline size_t ifo_row_bytes(const TxfShape& s) { return (sizeof(double) + 1) * (size_t)s.nfft + IFO_SCALAR_BYTES; }

inline int64_t ifo_chunk(const TxfShape& s, const TxfUse& u, int64_t frames_per_point, int64_t user_cap, size_t budget = TXF_WS_BUDGET) {
  return txf_chunk(s, u, frames_per_point, user_cap, budget, ifo_row_bytes(s));
}

// ---- the launch shape.  ifo_capture_kernel: a transform of Nfft / 8 threads per frame (fft_core.hpp's rule, restated;
// ofdm_ifo_study.hip asserts it): one workgroup per frame from Nfft 2048 on, and below that workgroups of 256 threads that hold
// 256 / (Nfft / 8) frames, so that no wavefront is launched part empty.  Static LDS: the padded exchange buffer of every transform
// and two words per wavefront for the search.  ifo_accumulate_kernel: the studies' accumulate launch (txf_plan.hpp:
// STUDY_ACC_*) over the Nfft bins, with the tail workgroup for the chunk's total errors.
constexpr int IFO_MAX_WAVES = 16;                    // Nfft 8192: 1024 threads

constexpr int ifo_threads(int nfft) { return nfft / 8 > 256 ? nfft / 8 : 256; }
constexpr int ifo_frames_per_wg(int nfft) { return ifo_threads(nfft) / (nfft / 8); }
constexpr size_t ifo_capture_lds(bool f64, int nfft) {
  return (size_t)(f64 ? 16 : 8) * ifo_frames_per_wg(nfft) * (size_t)(nfft + nfft / 8 + 8) + 2 * sizeof(int32_t) * IFO_MAX_WAVES;
}

// The largest case, double at Nfft 8192, is 147 712 bytes: inside the limit, one workgroup per CU.
static_assert(ifo_capture_lds(true, 8192) == 147712 && ifo_capture_lds(true, 8192) <= SYNC_LDS_LIMIT, "the capture kernel's LDS at its largest");
static_assert(ifo_capture_lds(true, 64) == 41088 &&ifo_capture_lds(true, 256) <= ifo_capture_lds(true, 64), "the small sizes pack 32 .. 2 frames");

struct IfoPass {
  int threads;               // per workgroup: max(256, Nfft / 8)
  int frames_per_wg;         // threads / (Nfft / 8)
  size_t lds;                // static LDS of the capture kernel
  unsigned grid;             // ceil(frames / frames_per_wg)
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // Nfft / STUDY_ACC_COLS + 1
  size_t acc_lds;            // static LDS of the accumulating kernel
};

inline IfoPass ifo_pass(const TxfShape& s, int64_t frames) {
  IfoPass p{};
  p.threads = ifo_threads(s.nfft);
  p.frames_per_wg = ifo_frames_per_wg(s.nfft);
  p.lds = ifo_capture_lds(s.f64 != 0, s.nfft);
  p.grid = (unsigned)((frames + p.frames_per_wg - 1) / p.frames_per_wg);
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(s.nfft, 1);
  p.acc_lds = STUDY_ACC_LDS;
  return p;
}

// ---- the two functions of a frame's scalars, one definition for the device code, the stand-alone program and (through it) the
// Python twins of tests/ifo_cases.py.
enum { IFO_ERR_BELOW = -1, IFO_ERR_ABOVE = -2 };

// The bin of the integer error d = IFO - rint(Freq_Shift), the frame's own draw rounded in double with ties to even: d + span in
// 0 .. 2 span, IFO_ERR_BELOW for d < -span, IFO_ERR_ABOVE for d > span (or a Freq_Shift that is not a number).  A difference of
// two integers held in doubles: exact, nothing a compiler can contract.
IFO_HD inline int ifo_err_bin(int32_t ifo, double cfo, int64_t span) {
  const double d = (double)ifo - ::rint(cfo);
  if (d < -(double)span) return IFO_ERR_BELOW;
  if (!(d <= (double)span)) return IFO_ERR_ABOVE;
  return (int)(d + (double)span);
}

// The total frequency error FreqOffset + IFO - Freq_Shift of T4/Main_model_Task_4.m:128-130, two rounded additions in this order.
IFO_HD inline double cfo_total_err(double freq_offset, int32_t ifo, double cfo) { return (freq_offset + (double)ifo) - cfo; }

}  // namespace ofdm
