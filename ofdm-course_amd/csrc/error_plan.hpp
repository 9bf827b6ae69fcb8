// The plan of one call of the error anatomy (ofdm_error_study.hip): ofdm_bit_error_profile, where the wrong bits of a batch of
// packed decisions sit against packed reference bits -- per data carrier, per OFDM symbol, per bit of the constellation label, the
// distances between neighbouring errors of a frame, per frame, and optionally on the time-frequency grid --, and ofdm_error_study,
// the same tables per point of a sweep of the fused generator decoded by the Task-5 or the Task-4 receiver.  The argument checks
// of both entries in the order they are made, the chunk the generator's workspace, the receiver's arena and the chunk's bit
// buffers allow, the launch shape with its LDS budget and the cap that keeps a workgroup's 32-bit counters from wrapping, and the
// function every layer shares: the position (OFDM symbol, data index, label bit) of stream bit i of a frame, the inverse of the
// pack stage (ofdm_chain.hip:323-339).  Plain C++ with no device or runtime dependency (ERR_HD is empty outside a device compile):
// tests/host/error_plan_main.cpp runs it under the host sanitizers against tests/error_cases.py.  The .hip side turns a refusal
// into OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "txf_plan.hpp"

#if defined(__HIPCC__)
#define ERR_HD __host__ __device__
#else
#define ERR_HD
#endif

namespace ofdm {

constexpr int ERR_MAX_GAP_BINS = 1024;
constexpr int ERR_MAX_BPS = 8;                        // 256QAM, the widest label the library maps
constexpr int64_t ERR_COUNTER_MAX = 0xffffffffll;     // a workgroup's LDS counters are uint32

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { ERR_REFUSE_FRAMES = TXF_REFUSALS, ERR_REFUSE_FRAME_BITS, ERR_REFUSE_RECEIVER, ERR_REFUSE_SIDE, ERR_REFUSE_TASK5_IMP,
       ERR_REFUSE_GAP_BINS, ERR_REFUSE_OUTPUT, ERR_REFUSALS };

// ---- the position of stream bit i of a frame: QAM index q = i / bps, label bit r = i % bps (MSB first), q = s nd + d
struct ErrPos {
  int64_t s;                 // OFDM symbol, 0-based
  int d;                     // index into dataCarriers, 0-based
  int r;                     // bit of the constellation label, 0 = MSB
};

ERR_HD inline ErrPos err_position(int64_t i, int nd, int bps) {
  const int64_t q = i / bps;
  return ErrPos{q / nd, (int)(q % nd), (int)(i % bps)};
}

// n / bps for 0 <= n < 64 and bps 1 .. 8 as a multiplication by err_recip(bps) = ceil(2^16 / bps): the product exceeds
// 2^16 n / bps by n e / bps with e < bps, and n e < 2^16 keeps that below the 1 / bps the quotient has to spare
ERR_HD inline uint32_t err_recip(int bps) { return (65536u + (uint32_t)bps - 1u) / (uint32_t)bps; }
ERR_HD inline int err_small_div(int n, uint32_t recip) { return (int)(((uint32_t)n * recip) >> 16); }

// the position `delta` (0 .. 32) stream bits behind p, without a division: what the kernel's per-bit loop runs
ERR_HD inline void err_advance(ErrPos& p, int delta, int nd, int bps, uint32_t recip) {
  const int r = p.r + delta;                          // < 8 + 32
  const int dq = err_small_div(r, recip);
  p.r = r - dq * bps;
  int64_t d = (int64_t)p.d + dq;
  while (d >= nd) { d -= nd; p.s += 1; }
  p.d = (int)d;
}

// ---- the tables of one call
struct ErrTablesWanted {
  int gap_bins = 0;
  bool out = false;          // an output is given
};

inline int64_t err_frame_bits(const TxfShape& s) { return (int64_t)s.nd * s.n_symb * s.bps; }

// The table checks, the last of both entries, in this order: the frame has at most 2^32 - 1 bits (frame_errors and a workgroup's
// counters are uint32) -> gap_bins 1 .. 1024 -> an output is given.
inline int err_check_tables(const TxfShape& s, const ErrTablesWanted& t, const char* what, TxfWhy& w) {
  if (!(err_frame_bits(s) <= ERR_COUNTER_MAX && s.bps >= 1 && s.bps <= ERR_MAX_BPS))
    return txf_refuse(w, ERR_REFUSE_FRAME_BITS, "%s: a frame must have at most 2^32 - 1 bits of 1 .. %d per symbol (%lld, %d)", what,
                      ERR_MAX_BPS, (long long)err_frame_bits(s), s.bps);
  if (!(t.gap_bins >= 1 && t.gap_bins <= ERR_MAX_GAP_BINS))
    return txf_refuse(w, ERR_REFUSE_GAP_BINS, "%s: gap_bins must be 1 .. %d (%d)", what, ERR_MAX_GAP_BINS, t.gap_bins);
  if (!t.out) return txf_refuse(w, ERR_REFUSE_OUTPUT, "%s: no output is given", what);
  return TXF_OK;
}

// ---- ofdm_bit_error_profile.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, bits, ref_bits) -> the plan's device -> the plan has data carriers -> n_frames 0 .. 2^31 - 1 -> the
//   tables (above).  Nothing else of the plan is read: any geometry the plan constructor accepts is accepted.
inline int err_profile_prelude(const TxfShape* plan, bool bits, bool ref_bits, int64_t n_frames, const ErrTablesWanted& t, TxfWhy& w) {
  static const char* const WHAT = "bit_error_profile";
  if (const int id = txf_check_args(plan && bits && ref_bits, WHAT, w)) return id;
  if (plan->device != plan->ctx_device)
    return txf_refuse(w, TXF_REFUSE_DEVICE, "RX plan belongs to device %d, the context is on device %d", plan->device, plan->ctx_device);
  if (plan->nd < 1) return txf_refuse(w, TXF_REFUSE_NO_DATA, "%s: the plan has no data carriers", WHAT);
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, ERR_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  return err_check_tables(*plan, t, WHAT, w);
}

// ---- ofdm_error_study.  c: the arguments as the matching sweep fills them (what = "ber_sweep_task5", "ber_sweep_task5_fading",
// "ber_sweep_task4" or "ber_sweep_task4_fading"; out and mp_desync set, no MER, no NMSE).  The order of its checks:
//   receiver 4 / 5 -> side 0 / 1 -> h and a tap-delay line together -> [receiver 5: sto_mode, cfo_mode, time_desync and
//   freq_desync are 0 and mp_desync is 1: ofdm_ber_sweep_task5 has none of them] -> the checks of the matching sweep, in its order
//   and its words (txf_task5_prelude / txf_task4_prelude: the generator's refusals among them) -> the tables (above)
struct ErrStudyArgs {
  int receiver = 5, side = 0;
  bool both_channels = false;
  int time_desync = 0, freq_desync = 0, mp_desync = 1;
};

inline int err_study_prelude(const TxfCall& c, const ErrStudyArgs& a, const ErrTablesWanted& t, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "error_study";
  if (!(a.receiver == 4 || a.receiver == 5))
    return txf_refuse(w, ERR_REFUSE_RECEIVER, "%s: receiver must be 4 (rx_chain_task4) or 5 (rx_chain_task5) (%d)", WHAT, a.receiver);
  if (!(a.side == 0 || a.side == 1))
    return txf_refuse(w, ERR_REFUSE_SIDE, "%s: side must be 0 (payload) or 1 (channel) (%d)", WHAT, a.side);
  if (a.both_channels)
    return txf_refuse(w, TXF_REFUSE_CHANNEL, "%s: give h (one channel for every frame) or taps (a channel per frame), not both", WHAT);
  if (a.receiver == 5) {
    if (!(c.sto_mode == 0 && c.cfo_mode == 0 && a.time_desync == 0 && a.freq_desync == 0 && a.mp_desync == 1))
      return txf_refuse(w, ERR_REFUSE_TASK5_IMP,
                        "%s: receiver 5 runs as ber_sweep_task5 does: no sto_mode / cfo_mode, time_desync and freq_desync 0, mp_desync 1", WHAT);
    if (const int id = txf_task5_prelude(c, ch, g, w)) return id;
  } else {
    if (const int id = txf_task4_prelude(c, ch, g, w)) return id;
  }
  return err_check_tables(*c.plan, t, WHAT, w);
}

// ---- the chunk of the study: frames of one point, budgeted as the matching sweep budgets its chunks (receiver 5: the generator's
// regions on the workspace budget; receiver 4: with the receiver's arena beside them, on twice that budget) and, beside them, per
// frame the two bit buffers of the study: the receiver's decisions and the scrambled reference, frame_words words each.
inline size_t err_bit_bytes(const TxfShape& s) { return 2 * sizeof(uint32_t) * (size_t)s.frame_words; }

inline TxfUse err_use(int receiver, bool scr, int fade_taps) {
  TxfUse u;
  u.scr = scr;
  u.sweep = true;
  u.imp = receiver == 4;     // the Task-4 sweep always draws (mode 0: zeros), and so does the study
  u.fade_taps = fade_taps;
  return u;
}

inline int64_t err_chunk(const TxfShape& s, const TxfUse& u, int receiver, int64_t frames_per_point, int64_t user_cap) {
  if (receiver == 4) {
    const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, 0, 0, 0, 0};
    return txf_chunk(s, u, frames_per_point, user_cap, 2 * TXF_WS_BUDGET, t4_frame_bytes(t4, s.frame_words) + err_bit_bytes(s));
  }
  return txf_chunk(s, u, frames_per_point, user_cap, TXF_WS_BUDGET, err_bit_bytes(s));
}

// ---- the launch shape of bit_error_profile_kernel.  Workgroups of ERR_THREADS threads; workgroup b walks the frames b, b + grid,
// ..; a frame is read in tiles of ERR_THREADS consecutive words, one word per thread.  Dynamic LDS, uint32 each: carrier[nd],
// symbol[N_symb], label[bps], gap[gap_bins + 1] (the last: the gaps above gap_bins), and ERR_SCRATCH_WORDS words of the scan (the
// wavefronts' last error positions, twice, as 64-bit values; the wavefronts' error counts).  The tables stay below ERR_LDS_LIMIT,
// the 64 KiB a kernel gets without asking: where symbol[N_symb] does not fit beside the others (N_symb beyond about 7000), the
// symbol counts go to the global table directly (symbols_in_lds = 0).
// The flush cap: a workgroup adds at most frame_bits to any of its counters per frame, so it may accumulate
// flush_frames = floor((2^32 - 1) / frame_bits) frames before it flushes (at least 1: the checks bound frame_bits).  A launch
// therefore takes at most grid * flush_frames frames; the host loops over launches.
constexpr int ERR_THREADS = 256;
constexpr int ERR_WAVES = ERR_THREADS / 64;
constexpr int ERR_MAX_GRID = 1024;
constexpr int ERR_SCRATCH_WORDS = 4 * ERR_WAVES + ERR_WAVES;
constexpr size_t ERR_LDS_LIMIT = 64 << 10;

struct ErrPass {
  int threads;               // ERR_THREADS
  int symbols_in_lds;
  size_t lds;                // dynamic LDS in bytes
  int64_t flush_frames;      // frames a workgroup accumulates before it flushes
  int64_t launch_frames;     // frames of one launch: min(frames, ERR_MAX_GRID * flush_frames)
  unsigned grid;             // min(launch_frames, ERR_MAX_GRID)
};

inline size_t err_lds_bytes(const TxfShape& s, int gap_bins, bool symbols) {
  return sizeof(uint32_t) * ((size_t)s.nd + (symbols ? (size_t)s.n_symb : 0) + (size_t)s.bps + (size_t)gap_bins + 1 + ERR_SCRATCH_WORDS);
}

inline ErrPass err_pass(const TxfShape& s, int gap_bins, int64_t frames) {
  ErrPass p{};
  p.threads = ERR_THREADS;
  p.symbols_in_lds = err_lds_bytes(s, gap_bins, true) <= ERR_LDS_LIMIT ? 1 : 0;
  p.lds = err_lds_bytes(s, gap_bins, p.symbols_in_lds != 0);
  p.flush_frames = std::max<int64_t>(1, ERR_COUNTER_MAX / std::max<int64_t>(1, err_frame_bits(s)));
  const int64_t most = p.flush_frames > ((int64_t)1 << 31) / ERR_MAX_GRID ? ((int64_t)1 << 31) : p.flush_frames * ERR_MAX_GRID;
  p.launch_frames = std::max<int64_t>(1, std::min<int64_t>(frames, most));
  p.grid = (unsigned)std::min<int64_t>(p.launch_frames, ERR_MAX_GRID);
  return p;
}

// the data carriers are distinct bins of an Nfft of at most 8192: without the symbol table the LDS always fits
static_assert(sizeof(uint32_t) * (8192 + ERR_MAX_BPS + ERR_MAX_GAP_BINS + 1 + ERR_SCRATCH_WORDS) <= ERR_LDS_LIMIT, "the tables of the largest Nfft fit");

}  // namespace ofdm
