// The plan of one call of the payload transport (ofdm_payload.hip): ofdm_tx_frames_payload, the fused frame generator with the
// caller's bits in place of the Philox payload, and ofdm_payload_transport, those frames at every point of a sweep decoded by the
// Task-5 or the Task-4 receiver and joined back into one stream.  What every driver of the reference does first: a picture's bits
// through the chain and back (T3/Main_model_Task_3.m:26-32, :160-185; file_reader.m, display_pic.m).  The argument checks of
// both entries in the order they are made, the number of frames of a payload, the chunk rule, the function every layer shares --
// where frame g of a call sits in the bit stream -- and the launch shapes.  Plain C++ with no device or runtime dependency (PAY_HD
// is empty outside a device compile): tests/host/payload_plan_main.cpp runs it under the host sanitizers against
// tests/payload_cases.py.  The .hip side turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text
// as the last-error string.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "txf_plan.hpp"

#if defined(__HIPCC__)
#define PAY_HD __host__ __device__
#else
#define PAY_HD
#endif

namespace ofdm {

constexpr int64_t PAY_STREAMS = (int64_t)1 << 32;     // the Philox streams of the generator: frame0 + n_frames < 2^32
constexpr int64_t PAY_MAX_FRAME_BITS = ((int64_t)1 << 31) - 1;   // frame_errors is uint32, a frame's bit index an int64 product

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { PAY_REFUSE_RECEIVER = TXF_REFUSALS, PAY_REFUSE_BITS, PAY_REFUSE_FIRST_FRAME, PAY_REFUSE_REPEATS, PAY_REFUSE_FRAMES,
       PAY_REFUSE_TASK5_IMP, PAY_REFUSE_FRAME_BITS, PAY_REFUSE_OUTPUT, PAY_REFUSALS };

// ---- the stream and its frames.  Stream bit i is bit 7 - i % 8 of byte i / 8.  A payload of n_bits is cut into
// F = ceil(n_bits / frame_bits) frames; frame k carries the stream bits k frame_bits .. k frame_bits + frame_bits - 1, those at or
// beyond n_bits are 0 (the padding display_pic.m:5-6 assumes).
PAY_HD inline int64_t payload_frames(int64_t n_bits, int64_t frame_bits) { return (n_bits + frame_bits - 1) / frame_bits; }

// Frame g of a call (0-based, in generation order) carries payload frame first_frame + g % period: the generator has no period
// (period = INT64_MAX: frame g is payload frame first_frame + g, beyond the payload all zeros); the transport sends the payload
// again for every repeat (first_frame = 0, period = F: frame g is repeat g / F, payload frame g % F).
struct PayloadCut {
  int64_t n_bits, frame_bits, first_frame, period;
};

struct PayloadPos {
  int64_t frame;             // the payload frame: first_frame + g % period
  int64_t repeat;            // g / period
  int64_t bit0;              // the stream bit of the frame's first bit, or -1: the frame lies beyond the payload
  int64_t share;             // how many of the frame's bits are payload: 0 .. frame_bits
};

PAY_HD inline PayloadPos payload_position(const PayloadCut& c, int64_t g) {
  PayloadPos p;
  p.repeat = g / c.period;
  p.frame = c.first_frame + (g - p.repeat * c.period);
  if (p.frame >= payload_frames(c.n_bits, c.frame_bits)) {     // (before the product: no overflow for a frame far outside)
    p.bit0 = -1;
    p.share = 0;
    return p;
  }
  p.bit0 = p.frame * c.frame_bits;
  const int64_t left = c.n_bits - p.bit0;
  p.share = left < c.frame_bits ? left : c.frame_bits;
  return p;
}

// how many of the 32 frame bits from frame bit i0 on are payload: 0 .. 32
PAY_HD inline int payload_valid(const PayloadPos& p, int64_t i0) {
  const int64_t v = p.share - i0;
  return v <= 0 ? 0 : v >= 32 ? 32 : (int)v;
}

// the words of a stream of n_bits, and of its staged copy: one zero word behind it, so that the funnel shift reads a pair
inline int64_t payload_words(int64_t n_bits) { return (n_bits + 31) / 32; }
inline int64_t payload_bytes(int64_t n_bits) { return (n_bits + 7) / 8; }
inline size_t payload_staged_bytes(int64_t n_bits) { return sizeof(uint32_t) * (size_t)(payload_words(n_bits) + 1); }

// ---- ofdm_tx_frames_payload.  c: the arguments as ofdm_tx_frames_fused_ex / _fading_ex fill them (what = "tx_frames_payload",
// with_imp, with_h or with_fading).  The order of its checks:
//   payload given and n_bits >= 1 -> first_frame 0 .. 2^32 - 1 -> h and a tap-delay line together -> the generator's checks, in
//   its order and words (txf_generator_prelude) -> the frame has at most 2^31 - 1 bits
inline int payload_check_frame_bits(const TxfShape& s, const char* what, TxfWhy& w) {
  const int64_t fb = (int64_t)s.nd * s.n_symb * s.bps;
  if (!(fb >= 1 && fb <= PAY_MAX_FRAME_BITS))
    return txf_refuse(w, PAY_REFUSE_FRAME_BITS, "%s: a frame must have 1 .. 2^31 - 1 bits (%lld)", what, (long long)fb);
  return TXF_OK;
}

inline int payload_generator_prelude(const TxfCall& c, bool payload, int64_t n_bits, int64_t first_frame, bool both_channels,
                                     TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "tx_frames_payload";
  if (!(payload && n_bits >= 1))
    return txf_refuse(w, PAY_REFUSE_BITS, "%s: the payload must have at least one bit (%lld)", WHAT, (long long)n_bits);
  if (!(first_frame >= 0 && first_frame < PAY_STREAMS))
    return txf_refuse(w, PAY_REFUSE_FIRST_FRAME, "%s: first_frame must be 0 .. 2^32 - 1 (%lld)", WHAT, (long long)first_frame);
  if (both_channels)
    return txf_refuse(w, TXF_REFUSE_CHANNEL, "%s: give h (one channel for every frame) or taps (a channel per frame), not both", WHAT);
  if (const int id = txf_generator_prelude(c, ch, g, w)) return id;
  return payload_check_frame_bits(*c.plan, WHAT, w);
}

// ---- ofdm_payload_transport.  c: the arguments as the matching sweep fills them, named "transport" (out and mp_desync set, no
// MER, no NMSE); its frames_per_point is set here, to F * repeats.  The order of its checks:
//   receiver 4 / 5 -> plan and payload given -> the plan has data carriers -> n_bits >= 1 -> repeats >= 1 -> F repeats and
//   frame0 + F repeats inside the generator's stream range -> h and a tap-delay line together -> [receiver 5: sto_mode, cfo_mode,
//   time_desync and freq_desync are 0 and mp_desync is 1: ofdm_ber_sweep_task5 has none of them] -> the checks of the matching
//   sweep in its order and its words (txf_task5_prelude / txf_task4_prelude: the generator's refusals, the Scrambler / DeScrambler
//   rule and the MMSE restriction among them) -> the frame has at most 2^31 - 1 bits -> an output is wanted
struct PayTransportArgs {
  int receiver = 5;
  bool payload = false, both_channels = false, out = false;
  int64_t n_bits = 0, repeats = 0;
  int time_desync = 0, freq_desync = 0, mp_desync = 1;
};

inline int payload_transport_prelude(TxfCall& c, const PayTransportArgs& a, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "transport";
  if (!(a.receiver == 4 || a.receiver == 5))
    return txf_refuse(w, PAY_REFUSE_RECEIVER, "%s: receiver must be 4 (rx_chain_task4) or 5 (rx_chain_task5) (%d)", WHAT, a.receiver);
  if (const int id = txf_check_args(c.plan && a.payload, WHAT, w)) return id;
  if (c.plan->nd < 1 || c.plan->n_symb < 1 || c.plan->bps < 1)
    return txf_refuse(w, TXF_REFUSE_NO_DATA, "%s: the plan has no data carriers", WHAT);
  if (!(a.n_bits >= 1)) return txf_refuse(w, PAY_REFUSE_BITS, "%s: the payload must have at least one bit (%lld)", WHAT, (long long)a.n_bits);
  if (!(a.repeats >= 1)) return txf_refuse(w, PAY_REFUSE_REPEATS, "%s: repeats must be at least 1 (%lld)", WHAT, (long long)a.repeats);
  const int64_t F = payload_frames(a.n_bits, (int64_t)c.plan->nd * c.plan->n_symb * c.plan->bps);
  // (no product before it is known to fit: F >= 1 here, and repeats <= (2^32 - 1 - frame0) / F is frame0 + F repeats < 2^32)
  if (!(F < PAY_STREAMS && c.frame0 >= 0 && c.frame0 < PAY_STREAMS && a.repeats <= (PAY_STREAMS - 1 - c.frame0) / F))
    return txf_refuse(w, PAY_REFUSE_FRAMES, "%s: %lld frames x %lld repeats from frame %lld leave the 32-bit stream range", WHAT,
                      (long long)F, (long long)a.repeats, (long long)c.frame0);
  c.n_frames = F * a.repeats;
  if (a.both_channels)
    return txf_refuse(w, TXF_REFUSE_CHANNEL, "%s: give h (one channel for every frame) or taps (a channel per frame), not both", WHAT);
  if (a.receiver == 5) {
    if (!(c.sto_mode == 0 && c.cfo_mode == 0 && a.time_desync == 0 && a.freq_desync == 0 && a.mp_desync == 1))
      return txf_refuse(w, PAY_REFUSE_TASK5_IMP,
                        "%s: receiver 5 runs as ber_sweep_task5 does: no sto_mode / cfo_mode, time_desync and freq_desync 0, mp_desync 1", WHAT);
    if (const int id = txf_task5_prelude(c, ch, g, w)) return id;
  } else {
    if (const int id = txf_task4_prelude(c, ch, g, w)) return id;
  }
  if (const int id = payload_check_frame_bits(*c.plan, WHAT, w)) return id;
  if (!a.out) return txf_refuse(w, PAY_REFUSE_OUTPUT, "%s: no output is wanted", WHAT);
  return TXF_OK;
}

// ---- the chunk of the transport: whole frames of one point, F * repeats of them in generation order, so a chunk may cut a repeat
// (and end inside an output word of the joined stream).  Budgeted as the matching sweep budgets its chunks (receiver 5: the
// generator's regions on the workspace budget; receiver 4: with the receiver's arena beside them, on twice that budget), with the
// payload's byte-per-bit region even without a Scrambler and, beside them, the receiver's decisions, frame_words words per frame.
inline size_t payload_bit_bytes(const TxfShape& s) { return sizeof(uint32_t) * (size_t)s.frame_words; }

inline TxfUse payload_use(int receiver, bool scr, int fade_taps) {
  TxfUse u;
  u.scr = scr;
  u.sweep = true;
  u.imp = receiver == 4;     // the Task-4 sweep always draws (mode 0: zeros), and so does the transport
  u.fade_taps = fade_taps;
  u.payload = true;
  return u;
}

inline int64_t payload_chunk(const TxfShape& s, const TxfUse& u, int receiver, int64_t frames, int64_t user_cap) {
  if (receiver == 4) {
    const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, 0, 0, 0, 0};
    return txf_chunk(s, u, frames, user_cap, 2 * TXF_WS_BUDGET, t4_frame_bytes(t4, s.frame_words) + payload_bit_bytes(s));
  }
  return txf_chunk(s, u, frames, user_cap, TXF_WS_BUDGET, payload_bit_bytes(s));
}

// ---- the launch shapes: workgroups of PAY_THREADS threads, at most PAY_MAX_GRID of them, every kernel a grid-stride loop.
//   payload_frames_kernel   item = one packed word of a frame (frame_words per frame), then one 16-byte group of the chunk's
//                           byte-per-bit region (ceil(nf frame_bits / 16); the region is padded to 256 bytes)
//   payload_join_kernel     item = one packed word of a frame's decisions
//   payload_tally_kernel    workgroup = one frame (its words summed in a fixed order), then, with `ones`, item = one stream bit
constexpr int PAY_THREADS = 256;
constexpr int64_t PAY_MAX_GRID = 4096;

inline int64_t payload_cut_items(const TxfShape& s, int64_t nf, bool ref) {
  const int64_t fb = (int64_t)s.nd * s.n_symb * s.bps;
  return (ref ? nf * s.frame_words : 0) + (nf * fb + 15) / 16;
}

inline unsigned payload_grid(int64_t items) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + PAY_THREADS - 1) / PAY_THREADS, PAY_MAX_GRID));
}

inline unsigned payload_tally_grid(int64_t nf, int64_t ones_bits) {
  return (unsigned)std::min<int64_t>(nf, PAY_MAX_GRID) + (ones_bits > 0 ? payload_grid(ones_bits) : 0u);
}

}  // namespace ofdm
