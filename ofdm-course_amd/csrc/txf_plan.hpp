// The plan of one call of the fused frame generator (ofdm_txfused.hip) or of a BER(SNR) sweep on top of it
// (ofdm_ber_sweep.hip): the channel of the call, the regions of the plan-owned workspace and the chunk they allow, the argument
// checks of the twelve entries in the order each entry makes them, and the launch shape of the channel pass -- decided before
// anything is launched or allocated.  Plain C++ with no device or runtime dependency: tests/host/txf_plan_main.cpp runs it
// under the host sanitizers against tests/txf_cases.py.  The .hip side turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE:
// OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "t4_route.hpp"      // t4_frame_bytes

namespace ofdm {

constexpr int TXF_MAX_TAPS = 64;
constexpr int TXF_MAX_DELAY = 4096;
constexpr int TXF_SEG = 4096;                       // output samples per channel workgroup
constexpr size_t TXF_WS_BUDGET = size_t(2) << 30;   // chunk cap of the plan-owned workspace
constexpr uint32_t TXF_DESCR_ON = 0x80000000u;      // = DESCR_ON (chain_fast_core.hpp)

struct TxfShape {            // what the generator and the sweeps read from the plan (and the context's device)
  int nfft, t_guard, n_symb, n_carrier, np, nd, bps, frame_words, f64, pilots_in_band;
  uint32_t descr;            // 0, or TXF_DESCR_ON | the DeScrambler register
  int mmse;                  // an MMSE operator is set (ofdm_rx_plan_set_mmse)
  int device, ctx_device;    // the plan's device and the context's
};

// ---- refusals: an id and the message, formatted into a fixed buffer
enum {
  TXF_OK = 0, TXF_REFUSE_ARGS, TXF_REFUSE_DEVICE, TXF_REFUSE_PRECISION, TXF_REFUSE_NO_DATA, TXF_REFUSE_PILOTS, TXF_REFUSE_NFFT,
  TXF_REFUSE_STREAM, TXF_REFUSE_MODES, TXF_REFUSE_SC_REF, TXF_REFUSE_CHANNEL, TXF_REFUSE_TAP_DELAY, TXF_REFUSE_TAP_COUNT,
  TXF_REFUSE_FADE_COUNT, TXF_REFUSE_FADE_MISSING, TXF_REFUSE_FADE_DELAY, TXF_REFUSE_FADE_TWICE, TXF_REFUSE_FADE_POWER,
  TXF_REFUSE_REGISTER, TXF_REFUSE_DESCR_NEEDED, TXF_REFUSE_DESCR_UNWANTED, TXF_REFUSE_POINTS_MISSING, TXF_REFUSE_POINTS_MANY,
  TXF_REFUSE_MMSE_POINTS, TXF_REFUSE_MMSE_FADING, TXF_REFUSE_CHUNK_CAP, TXF_REFUSE_MER_SKIP, TXF_REFUSE_NMSE_MP, TXF_REFUSALS
};

struct TxfWhy {
  char text[256] = "";
};

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline int txf_refuse(TxfWhy& w, int id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(w.text, sizeof(w.text), fmt, ap);
  va_end(ap);
  return id;
}

// ---- the channel of a call
struct TxfCx {
  double x, y;
};

struct TxfChannel {                                  // nonzero taps of h (conv_common's rule: exact zeros are skipped)
  std::vector<int32_t> delay;
  std::vector<TxfCx> amp;
  int halo = 0;                                      // largest delay: samples before a segment the FIR reaches back to
};

struct TxfGains {                                    // g_t = sqrt(tap_power[t] / sum tap_power), double (tx_fade_draw_kernel)
  double g[TXF_MAX_TAPS];
};

// a static h of h_len complex samples in the call's precision; null or empty: one unit tap (x * (1 + 0i) is exact)
inline int txf_channel(const void* h, int h_len, bool f64, TxfChannel& ch, TxfWhy& w) {
  if (!(h_len >= 0 && (h || h_len == 0))) return txf_refuse(w, TXF_REFUSE_CHANNEL, "tx_frames_fused: bad channel");
  if (!h || h_len == 0) {
    ch.delay.assign(1, 0);
    ch.amp.assign(1, TxfCx{1.0, 0.0});
    return TXF_OK;
  }
  for (int d = 0; d < h_len; ++d) {
    const double re = f64 ? ((const double*)h)[2 * (size_t)d] : ((const float*)h)[2 * (size_t)d];
    const double im = f64 ? ((const double*)h)[2 * (size_t)d + 1] : ((const float*)h)[2 * (size_t)d + 1];
    if (re != 0.0 || im != 0.0) {
      if (d > TXF_MAX_DELAY)
        return txf_refuse(w, TXF_REFUSE_TAP_DELAY, "tx_frames_fused: channel tap at delay %d (at most %d)", d, TXF_MAX_DELAY);
      ch.delay.push_back(d);
      ch.amp.push_back(TxfCx{re, im});
      ch.halo = d;
    }
  }
  if ((int)ch.delay.size() > TXF_MAX_TAPS)
    return txf_refuse(w, TXF_REFUSE_TAP_COUNT, "tx_frames_fused: %d nonzero channel taps (at most %d)", (int)ch.delay.size(),
                      TXF_MAX_TAPS);
  return TXF_OK;
}

// a per-frame channel on one tap-delay line: ch.delay / ch.halo as for a static h (ch.amp: the gains), the amplitudes are drawn
// per chunk.  The powers are summed in index order.
inline int txf_fading(const int32_t* tap_delay, const double* tap_power, int n_taps, const char* what, TxfChannel& ch,
                      TxfGains& gains, TxfWhy& w) {
  if (!(n_taps >= 1 && n_taps <= TXF_MAX_TAPS)) return txf_refuse(w, TXF_REFUSE_FADE_COUNT, "%s: n_taps must be 1 .. %d", what, TXF_MAX_TAPS);
  if (!(tap_delay && tap_power)) return txf_refuse(w, TXF_REFUSE_FADE_MISSING, "%s: tap_delay / tap_power missing", what);
  double total = 0;
  for (int t = 0; t < n_taps; ++t) {
    if (!(tap_delay[t] >= 0 && tap_delay[t] <= TXF_MAX_DELAY))
      return txf_refuse(w, TXF_REFUSE_FADE_DELAY, "%s: tap delay %d outside 0 .. %d", what, tap_delay[t], TXF_MAX_DELAY);
    for (int q = 0; q < t; ++q)
      if (tap_delay[q] == tap_delay[t]) return txf_refuse(w, TXF_REFUSE_FADE_TWICE, "%s: tap delay %d given twice", what, tap_delay[t]);
    if (!(tap_power[t] > 0.0 && std::isfinite(tap_power[t])))
      return txf_refuse(w, TXF_REFUSE_FADE_POWER, "%s: tap powers must be positive and finite", what);
    total += tap_power[t];
  }
  if (!std::isfinite(total)) return txf_refuse(w, TXF_REFUSE_FADE_POWER, "%s: tap powers must be positive and finite", what);
  gains = TxfGains{};
  for (int t = 0; t < n_taps; ++t) {
    gains.g[t] = std::sqrt(tap_power[t] / total);
    ch.delay.push_back(tap_delay[t]);
    ch.amp.push_back(TxfCx{gains.g[t], 0.0});
    ch.halo = std::max(ch.halo, (int)tap_delay[t]);
  }
  return TXF_OK;
}

// ---- the plan-owned workspace (pl->ws_txf): ONE table of its regions.  A region a call does not use has 0 bytes per frame.
enum { TXF_R_TX,            // the chunk's TX samples
       TXF_R_PARTIAL,       // sum |x|^2 per symbol, double
       TXF_R_B0, TXF_R_B1,  // Scrambler on: payload bits and scrambled bits, one byte each (B0 also for a caller's payload)
       TXF_R_RX, TXF_R_REF, // sweep: the chunk's RX frames and their packed reference bits
       TXF_R_STO, TXF_R_CFO,// impairments on: the chunk's draws (int64 / double)
       TXF_R_AMP,           // fading: the chunk's tap amplitudes [ch][fade_taps], complex double
       TXF_R_HEST,          // sweep with NMSE: the receiver's channel estimates [N_carrier x ch]
       TXF_REGIONS };

struct TxfUse {             // what a call needs of the workspace
  bool scr = false;         // the Scrambler register is given
  bool sweep = false;       // the frames are decoded in place (RX and reference bits stay in the workspace)
  bool imp = false;         // the Task-4 impairment draws
  int fade_taps = 0;        // > 0: a per-frame channel of that many taps
  bool hest = false;        // the receiver's channel estimates (sweep)
  bool payload = false;     // the caller's payload (payload_plan.hpp): its bits, one byte each, even without the Scrambler
};

struct TxfRegions {
  size_t per_frame[TXF_REGIONS];
};

inline TxfRegions txf_regions(const TxfShape& s, const TxfUse& u) {
  const size_t cs = s.f64 ? 16 : 8;
  const size_t fs = (size_t)(s.nfft + s.t_guard) * s.n_symb;
  const size_t frame_bits = (size_t)s.nd * s.n_symb * s.bps;
  TxfRegions r{};
  r.per_frame[TXF_R_TX] = cs * fs;
  r.per_frame[TXF_R_PARTIAL] = 8 * (size_t)s.n_symb;
  r.per_frame[TXF_R_B0] = u.scr || u.payload ? frame_bits : 0;
  r.per_frame[TXF_R_B1] = u.scr ? frame_bits : 0;
  r.per_frame[TXF_R_RX] = u.sweep ? cs * fs : 0;
  r.per_frame[TXF_R_REF] = u.sweep ? (size_t)s.frame_words * 4 : 0;
  r.per_frame[TXF_R_STO] = r.per_frame[TXF_R_CFO] = u.imp ? 8 : 0;
  r.per_frame[TXF_R_AMP] = 16 * (size_t)u.fade_taps;
  r.per_frame[TXF_R_HEST] = u.hest ? cs * (size_t)s.n_carrier : 0;
  return r;
}

// bytes per frame as the chunks are budgeted (no alignment padding)
inline size_t txf_frame_bytes(const TxfShape& s, const TxfUse& u) {
  const TxfRegions r = txf_regions(s, u);
  size_t b = 0;
  for (int i = 0; i < TXF_REGIONS; ++i) b += r.per_frame[i];
  return b;
}

struct TxfLayout {          // a chunk of ch frames: each region padded to 256 bytes, in the order of the table
  size_t off[TXF_REGIONS], bytes[TXF_REGIONS], total;
};

inline TxfLayout txf_layout(const TxfShape& s, const TxfUse& u, int64_t ch) {
  const TxfRegions r = txf_regions(s, u);
  TxfLayout l{};
  for (int i = 0; i < TXF_REGIONS; ++i) {
    l.off[i] = l.total;
    l.bytes[i] = (r.per_frame[i] * (size_t)ch + 255) & ~size_t(255);
    l.total += l.bytes[i];
  }
  return l;
}

// frames per chunk: the caller's cap, else what `budget` bytes hold of the workspace's frame and `extra` bytes beside it;
// at most the frames there are and the 65535 of a grid's y extent, at least 1
inline int64_t txf_chunk(const TxfShape& s, const TxfUse& u, int64_t n_frames, int64_t user_cap, size_t budget = TXF_WS_BUDGET,
                         size_t extra = 0) {
  const int64_t ch = user_cap > 0 ? user_cap : std::max<int64_t>(1, (int64_t)(budget / (txf_frame_bytes(s, u) + extra)));
  return std::max<int64_t>(1, std::min<int64_t>({ch, n_frames, 65535}));
}

// the Task-4 sweep: the generator workspace and the Task-4 arena (shared with ofdm_task5_part2_tile) budgeted together,
// + the per-frame MER sums when they are wanted
inline int64_t txf_chunk_task4(const TxfShape& s, const TxfUse& u, int64_t n_frames, int64_t user_cap, bool frame_mer) {
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, 0, 0, 0, 0};
  return txf_chunk(s, u, n_frames, user_cap, 2 * TXF_WS_BUDGET, t4_frame_bytes(t4, s.frame_words) + (frame_mer ? 16 : 0));
}

// ---- the accumulate stage of the studies (study_accumulate.hpp; hest_accumulate_kernel keeps the same shape): workgroups of
// STUDY_ACC_THREADS threads own STUDY_ACC_COLS columns of the chunk's rows each and stage STUDY_ACC_TILE rows at a time in LDS; where
// a study has per-frame scalars to sum, one more workgroup, the last, takes them.
constexpr size_t SYNC_LDS_LIMIT = 150 << 10;         // what every stage of this library keeps to
constexpr int STUDY_ACC_THREADS = 256;
constexpr int STUDY_ACC_COLS = 64;
constexpr int STUDY_ACC_TILE = 64;
constexpr size_t STUDY_ACC_LDS = sizeof(double) * STUDY_ACC_TILE * STUDY_ACC_COLS;

static_assert(STUDY_ACC_THREADS % STUDY_ACC_COLS == 0 && STUDY_ACC_TILE % (STUDY_ACC_THREADS / STUDY_ACC_COLS) == 0, "rows per thread and tile");
static_assert(STUDY_ACC_LDS == 32768 && STUDY_ACC_LDS <= SYNC_LDS_LIMIT, "the accumulating kernels' LDS");

// the workgroups of an accumulate launch: ceil(cols / STUDY_ACC_COLS), and `tail` (0 or 1) more for the per-frame scalars
inline unsigned study_acc_grid(int64_t cols, unsigned tail) { return (unsigned)((cols + STUDY_ACC_COLS - 1) / STUDY_ACC_COLS) + tail; }

// ---- the channel pass of a chunk of nf frames: one workgroup per (segment of TXF_SEG samples, frame)
enum { TXF_PASS_PLAIN, TXF_PASS_IMP, TXF_PASS_FADE, TXF_PASS_IMP_FADE };

struct TxfPass {
  int kernel;
  const char* name;
  int64_t len;              // samples per frame
  size_t lds;               // dynamic LDS: segment + halo (+ the frame's amplitudes behind them with fade)
  unsigned grid_x, grid_y;
};

inline TxfPass txf_channel_pass(const TxfShape& s, const TxfChannel& ch, bool imp, bool fade, int64_t nf) {
  static const char* const NAMES[] = {"tx_channel_fused_kernel", "tx_channel_imp_kernel", "tx_channel_fade_kernel",
                                      "tx_channel_imp_fade_kernel"};
  TxfPass p{};
  p.kernel = fade ? (imp ? TXF_PASS_IMP_FADE : TXF_PASS_FADE) : imp ? TXF_PASS_IMP : TXF_PASS_PLAIN;
  p.name = NAMES[p.kernel];
  p.len = (int64_t)(s.nfft + s.t_guard) * s.n_symb;
  p.lds = (s.f64 ? 16 : 8) * (size_t)(TXF_SEG + ch.halo + (fade ? ch.delay.size() : 0));
  p.grid_x = (unsigned)((p.len + TXF_SEG - 1) / TXF_SEG);
  p.grid_y = (unsigned)nf;
  return p;
}

// ---- the argument checks
inline int txf_check_args(bool ok, const char* what, TxfWhy& w) {
  return ok ? TXF_OK : txf_refuse(w, TXF_REFUSE_ARGS, "%s: bad arguments", what);
}

inline int txf_check_modes(int sto_mode, int cfo_mode, const char* what, TxfWhy& w) {
  if (sto_mode >= 0 && sto_mode <= 2 && cfo_mode >= 0 && cfo_mode <= 2) return TXF_OK;
  return txf_refuse(w, TXF_REFUSE_MODES, "%s: sto_mode / cfo_mode must be 0, 1 or 2", what);
}

// the sweeps' Scrambler rule: with the Scrambler on the plan descrambles with the same register, else not at all
inline int txf_check_descrambler(const TxfShape& s, const uint8_t* scr_reg15, const char* what, TxfWhy& w) {
  if (scr_reg15) {                                              // errors against the payload: the plan must descramble
    uint32_t d = TXF_DESCR_ON;
    for (int m = 1; m <= 14; ++m) {
      if (scr_reg15[m - 1] > 1) return txf_refuse(w, TXF_REFUSE_REGISTER, "%s: register entries must be 0 or 1", what);
      d |= (uint32_t)scr_reg15[m - 1] << (m - 1);
    }
    if (s.descr != d)
      return txf_refuse(w, TXF_REFUSE_DESCR_NEEDED, "%s: with the Scrambler on the plan needs a DeScrambler with the same register (ofdm_rx_plan_set_descrambler)", what);
  } else if (s.descr & TXF_DESCR_ON) {
    return txf_refuse(w, TXF_REFUSE_DESCR_UNWANTED, "%s: the plan descrambles but the frames are not scrambled", what);
  }
  return TXF_OK;
}

inline bool txf_nfft_ok(int n) { return n >= 64 && n <= 8192 && (n & (n - 1)) == 0; }   // = fft_size_ok (fft_core.hpp)

// the plan of a call, its precision flag and the Philox streams frame0 .. frame0 + n_frames - 1
inline int txf_check_plan(const TxfShape& s, bool f64_flag, int64_t frame0, int64_t n_frames, const char* what, TxfWhy& w) {
  if (s.device != s.ctx_device)
    return txf_refuse(w, TXF_REFUSE_DEVICE, "RX plan belongs to device %d, the context is on device %d", s.device, s.ctx_device);
  if ((f64_flag ? 1 : 0) != s.f64) return txf_refuse(w, TXF_REFUSE_PRECISION, "%s: precision flag differs from the plan's", what);
  if (s.nd < 1) return txf_refuse(w, TXF_REFUSE_NO_DATA, "%s: the plan has no data carriers", what);
  if (!s.pilots_in_band) return txf_refuse(w, TXF_REFUSE_PILOTS, "%s: pilots outside 1..N_carrier are not supported", what);
  if (!(txf_nfft_ok(s.nfft) && s.t_guard <= s.nfft))
    return txf_refuse(w, TXF_REFUSE_NFFT, "%s: unsupported Nfft %d / T_guard %d", what, s.nfft, s.t_guard);
  if (!(frame0 >= 0 && n_frames >= 0 && frame0 + n_frames < ((int64_t)1 << 32)))
    return txf_refuse(w, TXF_REFUSE_STREAM, "%s: frame index outside the 32-bit stream range", what);
  return TXF_OK;
}

// ---- the entries.  TxfCall: the arguments of an entry that its checks read; `what` names the entry in the messages.
struct TxfCall {
  const char* what = "";
  const TxfShape* plan = nullptr;                    // null: the entry was given no plan
  bool out = false;                                  // the mandatory output is given (rx_out; errors_out of a sweep)
  bool f64_flag = false;                             // the precision bit of `flags`
  int64_t frame0 = 0, n_frames = 0;                  // sweeps: n_frames = frames_per_point
  const uint8_t* scr_reg15 = nullptr;
  bool fading = false;                               // the channel: a tap-delay line (below), else a static h
  const void* h = nullptr;
  int h_len = 0;
  const int32_t* tap_delay = nullptr;
  const double* tap_power = nullptr;
  int n_taps = 0;
  bool imp = false;                                  // the entry takes impairments: sto_mode / cfo_mode
  int sto_mode = 0, cfo_mode = 0;
  bool sc_ref_out = false;                           // generator: sc_ref_bits_out is given
  const double* snr_db = nullptr;                    // sweeps
  const uint64_t* seeds = nullptr;
  int64_t n_points = 0, max_chunk = 0;
  int64_t mer_skip = 0;                              // Task-4 sweeps
  bool nmse_out = false;                             // Task-4 sweeps: nmse_sums_out or frame_nmse_out is given
  int mp_desync = 0;

  TxfCall(const char* what_, int64_t frame0_, int64_t n_frames_, const uint8_t* scr_reg15_)
      : what(what_), frame0(frame0_), n_frames(n_frames_), scr_reg15(scr_reg15_) {}
  TxfCall& with_h(const void* h_, int h_len_) { h = h_; h_len = h_len_; return *this; }
  TxfCall& with_fading(const int32_t* tap_delay_, const double* tap_power_, int n_taps_) {
    fading = true; tap_delay = tap_delay_; tap_power = tap_power_; n_taps = n_taps_; return *this;
  }
  TxfCall& with_imp(int sto_mode_, int cfo_mode_) { imp = true; sto_mode = sto_mode_; cfo_mode = cfo_mode_; return *this; }
  TxfCall& with_points(const double* snr_db_, const uint64_t* seeds_, int64_t n_points_, int64_t max_chunk_) {
    snr_db = snr_db_; seeds = seeds_; n_points = n_points_; max_chunk = max_chunk_; return *this;
  }
};

// the channel of the call; a static h is read in precision f64 and refused in the words of tx_frames_fused, whatever the entry
inline int txf_call_channel(const TxfCall& c, bool f64, const char* what, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  return c.fading ? txf_fading(c.tap_delay, c.tap_power, c.n_taps, what, ch, g, w) : txf_channel(c.h, c.h_len, f64, ch, w);
}

// the checks all sweeps make on their points and the plan
inline int txf_check_sweep(const TxfCall& c, const char* what, TxfWhy& w) {
  if (!(c.n_points == 0 || (c.snr_db && c.seeds))) return txf_refuse(w, TXF_REFUSE_POINTS_MISSING, "%s: snr_db / seeds missing", what);
  if (!(c.n_points < ((int64_t)1 << 31))) return txf_refuse(w, TXF_REFUSE_POINTS_MANY, "%s: too many points", what);
  return txf_check_plan(*c.plan, c.f64_flag, c.frame0, c.n_frames, what, w);
}

// The order of the checks of every entry; the first that fails is the refusal a caller sees.
//
// ofdm_tx_frames_fused / _fading / _fused_ex / _fading_ex (what = the entry's name without "ofdm_"):
//   bad arguments (plan, n_frames >= 0, rx_out) -> the plan (device, precision, data carriers, pilots in band, Nfft / T_guard,
//   stream range) -> [_ex: sto_mode / cfo_mode] -> sc_ref_bits_out needs the register -> the channel (h: bad channel, tap delay,
//   tap count, always as "tx_frames_fused"; fading: n_taps, pointers, then per tap delay range, duplicate, power; the sum)
inline int txf_generator_prelude(const TxfCall& c, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  if (const int id = txf_check_args(c.plan && c.n_frames >= 0 && c.out, c.what, w)) return id;
  if (const int id = txf_check_plan(*c.plan, c.f64_flag, c.frame0, c.n_frames, c.what, w)) return id;
  if (c.imp)
    if (const int id = txf_check_modes(c.sto_mode, c.cfo_mode, c.what, w)) return id;
  if (!(c.scr_reg15 || !c.sc_ref_out)) return txf_refuse(w, TXF_REFUSE_SC_REF, "%s: sc_ref_bits_out needs the Scrambler register", c.what);
  return txf_call_channel(c, c.plan->f64 != 0, c.what, ch, g, w);
}

// ofdm_ber_sweep_task5 / _task5_ex (what = "ber_sweep_task5") and ofdm_ber_sweep_task5_fading (what = "ber_sweep_task5_fading"):
//   bad arguments (plan, n_points >= 0, frames_per_point >= 0, max_frames_per_chunk >= 0, errors_out) -> snr_db / seeds ->
//   too many points -> the plan (as above, the streams of one point) -> the MMSE restriction (static: one point; fading: none
//   at all) -> the Scrambler / DeScrambler rule (register entries, same register, or no DeScrambler) -> the channel (as above)
inline int txf_task5_prelude(const TxfCall& c, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  if (const int id = txf_check_args(c.plan && c.n_points >= 0 && c.n_frames >= 0 && c.max_chunk >= 0 && c.out, c.what, w)) return id;
  if (const int id = txf_check_sweep(c, c.what, w)) return id;
  if (c.fading) {
    if (c.plan->mmse)
      return txf_refuse(w, TXF_REFUSE_MMSE_FADING, "%s: an MMSE-mode plan is built for one channel h (ofdm_rx_plan_set_mmse)", c.what);
  } else if (c.plan->mmse && c.n_points > 1) {
    return txf_refuse(w, TXF_REFUSE_MMSE_POINTS, "%s: an MMSE-mode plan is built for one SNR (n_points must be 1)", c.what);
  }
  if (const int id = txf_check_descrambler(*c.plan, c.scr_reg15, c.what, w)) return id;
  return txf_call_channel(c, c.plan->f64 != 0, c.what, ch, g, w);
}

// ofdm_ber_sweep_task4 / _ex / _nmse (what = "ber_sweep_task4") and ofdm_ber_sweep_task4_fading (what = "ber_sweep_task4_fading"
// up to the channel, "ber_sweep_task4" behind it):
//   bad arguments (plan, n_points >= 0, frames_per_point >= 0, errors_out) -> the channel (a static h read in the precision of
//   `flags`: the plan has not been looked at yet) -> max_frames_per_chunk 0..65535 -> snr_db / seeds -> too many points -> the
//   plan -> sto_mode / cfo_mode -> the Scrambler / DeScrambler rule -> mer_skip -> the NMSE outputs need mp_desync
inline int txf_task4_prelude(const TxfCall& c, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const T4 = "ber_sweep_task4";
  if (const int id = txf_check_args(c.plan && c.n_points >= 0 && c.n_frames >= 0 && c.out, c.what, w)) return id;
  if (const int id = txf_call_channel(c, c.f64_flag, c.what, ch, g, w)) return id;
  if (!(c.max_chunk >= 0 && c.max_chunk <= 65535))
    return txf_refuse(w, TXF_REFUSE_CHUNK_CAP, "ber_sweep_task4: max_frames_per_chunk must be 0..65535 (the limit of rx_chain_task4)");
  if (const int id = txf_check_sweep(c, T4, w)) return id;
  if (const int id = txf_check_modes(c.sto_mode, c.cfo_mode, T4, w)) return id;
  if (const int id = txf_check_descrambler(*c.plan, c.scr_reg15, T4, w)) return id;
  if (!(c.mer_skip >= 0 && c.mer_skip < (int64_t)c.plan->nd * c.plan->n_symb))
    return txf_refuse(w, TXF_REFUSE_MER_SKIP, "ber_sweep_task4_ex: mer_skip must be 0 .. nd * N_symb - 1 (%lld)", (long long)c.mer_skip);
  if (c.nmse_out && !c.mp_desync)
    return txf_refuse(w, TXF_REFUSE_NMSE_MP, "ber_sweep_task4: the NMSE outputs need mp_desync (without estimate_channel there is no estimate)");
  return TXF_OK;
}

// ---- the studies (ofdm_spectrum_study, _sync_study, _fine_study, _ifo_study, _hest_study): one device-resident call that generates
// the frames of every point of a sweep and runs part of a receiver on them.
// The front of a study's checks, in this order; the study's own capture checks follow it.  c: the generator arguments as the sweeps
// fill them (n_frames = frames_per_point, with_points, with_imp, with_h or with_fading); both_channels: h and a tap-delay line are
// given, refused with the study's own id refuse_both; chunk_cap: the largest max_frames_per_chunk the study takes (65535 behind
// the Task-4 receiver).
//   bad arguments (plan, n_points >= 0, frames_per_point >= 0, max_frames_per_chunk 0 .. chunk_cap) -> snr_db / seeds -> too many
//   points -> the plan (the streams of one point) -> sto_mode / cfo_mode -> register entries 0 / 1 -> h and taps together -> the
//   channel (h: bad channel, tap delay, tap count, as "tx_frames_fused"; taps: n_taps, pointers, per tap delay range, duplicate,
//   power; the sum)
inline int txf_study_prelude(const TxfCall& c, bool both_channels, int refuse_both, const char* what, TxfChannel& ch, TxfGains& g,
                             TxfWhy& w, int64_t chunk_cap = INT64_MAX) {
  if (const int id = txf_check_args(c.plan && c.n_points >= 0 && c.n_frames >= 0 && c.max_chunk >= 0 && c.max_chunk <= chunk_cap, what, w))
    return id;
  if (const int id = txf_check_sweep(c, what, w)) return id;
  if (const int id = txf_check_modes(c.sto_mode, c.cfo_mode, what, w)) return id;
  if (c.scr_reg15)
    for (int m = 0; m < 15; ++m)
      if (c.scr_reg15[m] > 1) return txf_refuse(w, TXF_REFUSE_REGISTER, "%s: register entries must be 0 or 1", what);
  if (both_channels) return txf_refuse(w, refuse_both, "%s: give h (one channel for every frame) or taps (a channel per frame), not both", what);
  return txf_call_channel(c, c.plan->f64 != 0, what, ch, g, w);
}

// what a study needs of the workspace: the generator's regions with the RX region (the frames stay in the workspace, where the
// capture reads them)
inline TxfUse txf_study_use(bool scr, bool imp, int fade_taps) {
  TxfUse u;
  u.scr = scr;
  u.sweep = true;
  u.imp = imp;
  u.fade_taps = fade_taps;
  return u;
}

}  // namespace ofdm
