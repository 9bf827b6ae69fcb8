// The plan of one call of the Task-2 PAPR / CCDF study (ofdm_papr_study, ofdm_papr_study.hip; T2/Main_model_Task_2.m:69-97 over
// many signals): the bin of a value, the argument checks of the entry in the order they are made, the chunk of whole signals the
// generator's workspace allows and the launch shape of the histogram pass -- decided before anything is launched or allocated.
// Plain C++ with no device or runtime dependency: tests/host/papr_plan_main.cpp runs it under the host sanitizers against
// tests/papr_cases.py.  papr_bin is the one function that bins, on the device (papr_hist_kernel) and on the host: OFDM_PAPR_HD is
// the device qualifier where the device compiler reads this file and empty elsewhere.  The .hip side turns a refusal into
// OFDM_ERR_ARG (PAPR_REFUSE_DEVICE: OFDM_ERR_STATE) with PaprWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "txf_plan.hpp"      // TxfShape, TxfUse, txf_frame_bytes, txf_check_plan, TXF_WS_BUDGET

#if defined(__HIPCC__)
#define OFDM_PAPR_HD __host__ __device__
#else
#define OFDM_PAPR_HD
#endif

namespace ofdm {

constexpr int PAPR_MAX_BINS = 4096;
constexpr int PAPR_MIN_WINDOW = 256;
constexpr int PAPR_MAX_WINDOW = 8192;
constexpr int PAPR_TAILS = 3;                        // below lo, at or above hi, NaN
constexpr size_t PAPR_LDS_LIMIT = size_t(160) << 10; // the LDS of a CU
constexpr size_t PAPR_STATIC_LDS = 256;              // papr_hist_kernel's wave totals (2 x 16 doubles)
constexpr int64_t PAPR_MAX_SIGNALS_PER_CHUNK = 65535;// a grid's y extent

enum { PAPR_OK = 0, PAPR_REFUSE_ARGS, PAPR_REFUSE_DEVICE, PAPR_REFUSE_PRECISION, PAPR_REFUSE_NO_DATA, PAPR_REFUSE_PILOTS,
       PAPR_REFUSE_NFFT, PAPR_REFUSE_STREAM, PAPR_REFUSE_SIGNALS, PAPR_REFUSE_FRAMES, PAPR_REFUSE_BINS, PAPR_REFUSE_RANGE,
       PAPR_REFUSE_WINDOW, PAPR_REFUSE_WINDOW_LONG, PAPR_REFUSE_REGISTER, PAPR_REFUSE_CHUNK_CAP, PAPR_REFUSE_LDS, PAPR_REFUSALS };

struct PaprWhy {
  char text[256] = "";
};

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline int papr_refuse(PaprWhy& w, int id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(w.text, sizeof(w.text), fmt, ap);
  va_end(ap);
  return id;
}

// The bin of one window value v (dB), double arithmetic: 0 .. n_bins - 1 = floor((v - lo_db) * n_bins / (hi_db - lo_db)) for
// lo_db <= v < hi_db; n_bins + 0 for v < lo_db (-Inf included), n_bins + 1 for v >= hi_db (+Inf included), n_bins + 2 for NaN
// (the 0 / 0 of an all-zero window, calculatePAPR.m:4-10).  The tails are decided on v itself, before the product is formed; a
// v one rounding below hi_db whose quotient rounds up to n_bins stays in the last bin.
OFDM_PAPR_HD inline int papr_bin(double v, double lo_db, double hi_db, int n_bins) {
  if (v != v) return n_bins + 2;
  if (v < lo_db) return n_bins;
  if (v >= hi_db) return n_bins + 1;
  const double t = floor((v - lo_db) * (double)n_bins / (hi_db - lo_db));
  if (!(t >= 0.0)) return 0;
  if (t >= (double)n_bins) return n_bins - 1;
  return (int)t;
}

inline bool papr_window_ok(int w) { return w >= PAPR_MIN_WINDOW && w <= PAPR_MAX_WINDOW && (w & (w - 1)) == 0; }

// ---- the launch shape of the histogram pass: a workgroup owns `window` consecutive window starts of one signal
struct PaprPass {
  int threads;              // 128 .. 1024, window_papr_reg_kernel's
  int per_thread;           // C = 2 * window / threads samples per thread: 4, 8 or 16
  bool two_phase;           // window 8192: one pair of scan arrays for the maxima, then the sums
  size_t scan_bytes;        // the scan arrays, doubles
  size_t lds;               // dynamic LDS: the scan arrays, then n_bins + PAPR_TAILS uint32 counts
  int64_t windows;          // per signal: frames_per_signal * frame_samples - window + 1
  unsigned grid_x, grid_y;  // (workgroups per signal, signals of the chunk)
};

inline PaprPass papr_pass(int window, int n_bins, int64_t signal_samples, int64_t signals_in_chunk) {
  PaprPass p{};
  p.threads = window == 256 ? 128 : window <= 1024 ? 256 : window == 2048 ? 512 : 1024;
  p.per_thread = 2 * window / p.threads;
  p.two_phase = window == 8192;
  p.scan_bytes = sizeof(double) * (size_t)(window + (window >> 5) + 1) * (p.two_phase ? 2 : 4);
  p.lds = p.scan_bytes + sizeof(uint32_t) * (size_t)(n_bins + PAPR_TAILS);
  p.windows = signal_samples - window + 1;
  p.grid_x = (unsigned)((p.windows + window - 1) / window);
  p.grid_y = (unsigned)signals_in_chunk;
  return p;
}

// ---- the chunk: whole signals, budgeted on the generator's regions with no RX region (txf_plan.hpp); the caller's cap counts
// frames and is rounded down to whole signals; at least one signal, at most the signals there are and a grid's y extent
inline TxfUse papr_use(bool scr) {
  TxfUse u;
  u.scr = scr;
  return u;
}

inline int64_t papr_chunk_signals(const TxfShape& s, bool scr, int64_t n_signals, int frames_per_signal, int64_t user_cap,
                                  size_t budget = TXF_WS_BUDGET) {
  const int64_t frames = user_cap > 0 ? user_cap : (int64_t)(budget / txf_frame_bytes(s, papr_use(scr)));
  return std::max<int64_t>(1, std::min<int64_t>({frames / frames_per_signal, n_signals, PAPR_MAX_SIGNALS_PER_CHUNK}));
}

// ---- the entry.  PaprCall: the arguments of ofdm_papr_study that its checks read.
struct PaprCall {
  const TxfShape* plan = nullptr;                    // null: the entry was given no plan
  bool out = false;                                  // hist_out and tails_out are given
  bool f64_flag = false;                             // the precision bit of `flags`
  int64_t frame0 = 0, n_signals = 0;
  int frames_per_signal = 0;
  const uint8_t* scr_reg15 = nullptr;
  int window = 0, n_bins = 0;
  double lo_db = 0, hi_db = 0;
  int64_t max_chunk = 0;
};

// The order of the checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, hist_out, tails_out) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in
//   band, Nfft / T_guard, frame0 in the stream range) -> n_signals >= 0 -> frames_per_signal >= 1 -> the stream range of all
//   n_signals * frames_per_signal frames -> n_bins 1 .. 4096 -> lo_db < hi_db, both finite -> window a power of two 256 .. 8192
//   -> window <= frames_per_signal * frame_samples -> register entries 0 / 1 -> max_frames_per_chunk >= 0 -> the LDS of the
//   histogram pass within 160 KB
inline int papr_prelude(const PaprCall& c, PaprWhy& w) {
  static const char* const WHAT = "papr_study";
  if (!(c.plan && c.out)) return papr_refuse(w, PAPR_REFUSE_ARGS, "papr_study: bad arguments");
  const TxfShape& s = *c.plan;
  TxfWhy tw;
  if (const int id = txf_check_plan(s, c.f64_flag, c.frame0, 0, WHAT, tw)) {
    static const int MAP[] = {PAPR_OK, PAPR_REFUSE_ARGS, PAPR_REFUSE_DEVICE, PAPR_REFUSE_PRECISION, PAPR_REFUSE_NO_DATA,
                              PAPR_REFUSE_PILOTS, PAPR_REFUSE_NFFT, PAPR_REFUSE_STREAM};
    std::snprintf(w.text, sizeof(w.text), "%s", tw.text);
    return id <= TXF_REFUSE_STREAM ? MAP[id] : PAPR_REFUSE_ARGS;
  }
  if (!(c.n_signals >= 0)) return papr_refuse(w, PAPR_REFUSE_SIGNALS, "papr_study: n_signals must be >= 0 (%lld)", (long long)c.n_signals);
  if (!(c.frames_per_signal >= 1))
    return papr_refuse(w, PAPR_REFUSE_FRAMES, "papr_study: frames_per_signal must be >= 1 (%d)", c.frames_per_signal);
  // compared without forming n_signals * frames_per_signal, which may not fit 64 bits
  if (c.n_signals > (((int64_t)1 << 32) - 1 - c.frame0) / c.frames_per_signal)
    return papr_refuse(w, PAPR_REFUSE_STREAM, "papr_study: frame index outside the 32-bit stream range");
  if (!(c.n_bins >= 1 && c.n_bins <= PAPR_MAX_BINS))
    return papr_refuse(w, PAPR_REFUSE_BINS, "papr_study: n_bins must be 1 .. %d (%d)", PAPR_MAX_BINS, c.n_bins);
  if (!(std::isfinite(c.lo_db) && std::isfinite(c.hi_db) && c.lo_db < c.hi_db))
    return papr_refuse(w, PAPR_REFUSE_RANGE, "papr_study: lo_db and hi_db must be finite with lo_db < hi_db");
  if (!papr_window_ok(c.window))
    return papr_refuse(w, PAPR_REFUSE_WINDOW, "papr_study: window must be a power of two, %d .. %d (%d)", PAPR_MIN_WINDOW,
                       PAPR_MAX_WINDOW, c.window);
  const int64_t signal_samples = (int64_t)c.frames_per_signal * (s.nfft + s.t_guard) * s.n_symb;
  if (c.window > signal_samples)
    return papr_refuse(w, PAPR_REFUSE_WINDOW_LONG, "papr_study: window %d exceeds the signal of %lld samples", c.window,
                       (long long)signal_samples);
  if (c.scr_reg15)
    for (int m = 0; m < 15; ++m)
      if (c.scr_reg15[m] > 1) return papr_refuse(w, PAPR_REFUSE_REGISTER, "papr_study: register entries must be 0 or 1");
  if (!(c.max_chunk >= 0)) return papr_refuse(w, PAPR_REFUSE_CHUNK_CAP, "papr_study: max_frames_per_chunk must be >= 0");
  const PaprPass p = papr_pass(c.window, c.n_bins, signal_samples, 1);
  if (p.lds + PAPR_STATIC_LDS > PAPR_LDS_LIMIT)
    return papr_refuse(w, PAPR_REFUSE_LDS, "papr_study: the histogram pass needs %zu bytes of LDS (at most %zu)",
                       p.lds + PAPR_STATIC_LDS, (size_t)PAPR_LDS_LIMIT);
  return PAPR_OK;
}

}  // namespace ofdm
