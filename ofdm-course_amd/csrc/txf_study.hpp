// The scaffold of a sweep or a study on the fused frame generator, HIP side: the point x chunk loop with the generation inside
// (txf_sweep_points; its bit source the Philox draw or, for the transport, the caller's stream), the generator arguments every study entry takes (TxfStudyArgs), and the two ways a study stages an output: an
// accumulator table (txf_table) and a per-frame array (TxfFrameOut).  What a call decides -- its checks, its channel, its chunk --
// is txf_plan.hpp's (txf_study_prelude, txf_study_use) and the study's own plan header's.
#pragma once

#include <algorithm>
#include <cmath>

#include "txf_generate.hpp"

namespace ofdm {

// the points of a sweep: point p at snr_db[p] with the Philox key seeds[p], frames frame0 .. frame0 + frames_per_point - 1
struct TxfPoints {
  const double* snr_db;
  const uint64_t* seeds;
  int64_t n_points, frames_per_point, frame0;
  bool ref = true;             // the chunk's packed payload bits go to b.ref (false: nothing compares them, they are not written)
  uint32_t* scref = nullptr;   // the chunk's packed scrambled bits (the error study's channel side)
  const TxfPayload* payload = nullptr;   // the frames' bits from the caller's stream (the transport); null: the Philox draw
};

// every point of a sweep, chunk by chunk of at most CH frames: the chunk generated into the workspace, then body(b, nf, p, o) with
// o = p * frames_per_point + c0 the sweep index of the chunk's first frame.  imp: with the Task-4 impairments, the draws of the
// chunk's frames at imp->sto + o / imp->cfo + o (arrays over the whole sweep), or, where imp->sto is null, at the chunk's own
// b.sto / b.cfo; fade: with a channel per frame, the chunk's amplitudes at b.amp.  u: the workspace's regions.
template <typename Body>
int txf_sweep_points(ofdm_rx_plan* pl, const TxfChannel& ch, const TxfPoints& pt, const uint8_t* scr_reg15, int64_t CH,
                     const TxfImp* imp, const TxfFade* fade, const TxfUse& u, Body&& body) {
  OFDM_TRY(tx_dict_device(pl));
  TxfBuffers b;
  OFDM_TRY(txf_workspace(pl, CH, u, b));
  TxfImp ci;
  if (imp) ci = *imp;
  ci.sto = b.sto;
  ci.cfo = b.cfo;
  TxfFade cf;
  if (fade) cf = *fade;
  cf.amp = b.amp;
  TxfPayload cp;
  if (pt.payload) cp = *pt.payload;
  for (int64_t p = 0; p < pt.n_points; ++p) {
    const double snr_lin = std::pow(10.0, pt.snr_db[p] / 10.0);
    const uint32_t k0 = (uint32_t)pt.seeds[p], k1 = (uint32_t)(pt.seeds[p] >> 32);
    for (int64_t c0 = 0; c0 < pt.frames_per_point; c0 += CH) {
      const int64_t nf = std::min<int64_t>(CH, pt.frames_per_point - c0);
      const int64_t o = p * pt.frames_per_point + c0;
      if (imp && imp->sto) { ci.sto = imp->sto + o; ci.cfo = imp->cfo + o; }
      cp.frame = c0;
      OFDM_TRY(txf_generate(pl, ch, snr_lin, k0, k1, (uint32_t)(pt.frame0 + c0), nf, scr_reg15, b, b.rx, pt.ref ? b.ref : nullptr,
                            pt.scref, imp ? &ci : nullptr, fade ? &cf : nullptr, pt.payload ? &cp : nullptr));
      OFDM_TRY(body(b, nf, p, o));
    }
  }
  return OFDM_OK;
}

// the generator arguments of a study entry, in the order the entries take them
struct TxfStudyArgs {
  const void* h;
  int h_len;
  const int32_t* tap_delay;
  const double* tap_power;
  int n_taps, sto_mode;
  int64_t sto_value;
  int cfo_mode;
  double cfo_value;
  const uint8_t* scr_reg15;
  const double* snr_db;
  const uint64_t* seeds;
  int64_t n_points, frames_per_point, frame0, max_frames_per_chunk;
  int flags;

  bool fading() const { return tap_delay || tap_power || n_taps != 0; }
  bool both_channels() const { return fading() && h && h_len != 0; }
  bool imp_on() const { return sto_mode != 0 || cfo_mode != 0; }    // both off: the plain channel pass, the same frames
  // what the study's checks read: the call named `what` on the plan's shape (null: the entry was given no plan)
  TxfCall call(const char* what, const TxfShape* plan) const {
    TxfCall c(what, frame0, frames_per_point, scr_reg15);
    c.plan = plan;
    c.f64_flag = is_f64(flags);
    c.with_points(snr_db, seeds, n_points, max_frames_per_chunk).with_imp(sto_mode, cfo_mode);
    if (fading()) c.with_fading(tap_delay, tap_power, n_taps);
    else c.with_h(h, h_len);
    return c;
  }
  TxfImp imp() const { return TxfImp(sto_mode, sto_value, cfo_mode, cfo_value); }   // the draws: the chunk's own (txf_sweep_points)
  TxfPoints points(bool ref = false) const { return TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0, ref}; }
  TxfUse use(const TxfChannel& ch) const { return txf_study_use(scr_reg15 != nullptr, imp_on(), fading() ? (int)ch.delay.size() : 0); }
};

// an accumulator table of n elements: the caller's, or scratch where the caller wants none (the tables nobody asked for are still
// counted: one kernel, whatever the outputs); zeroed on the launch stream: 0 + v_0 + v_1 + ..
template <typename D, typename U>
int txf_table(Stage& st, U* user, size_t n, D*& d) {
  static_assert(sizeof(D) == sizeof(U), "the table's element as the caller and the kernel name it");
  void* v = nullptr;
  OFDM_TRY(user ? st.out(user, sizeof(D) * n, &v) : st.scratch(sizeof(D) * n, &v));
  OFDM_HIP(hipMemsetAsync(v, 0, sizeof(D) * n, ctx().stream));
  d = (D*)v;
  return OFDM_OK;
}

// a per-frame output: the caller's array over the whole sweep, written at the sweep index of a chunk's first frame, or scratch
// for one chunk
template <typename T>
struct TxfFrameOut {
  T *sweep = nullptr, *chunk = nullptr;
  int out(Stage& st, T* user, size_t n_sweep) {
    void* v = nullptr;
    OFDM_TRY(st.out(user, sizeof(T) * n_sweep, &v));
    sweep = (T*)v;
    return OFDM_OK;
  }
  int scratch(Stage& st, size_t n_chunk) {             // nothing where the caller's array is staged
    void* v = nullptr;
    if (!sweep) OFDM_TRY(st.scratch(sizeof(T) * n_chunk, &v));
    chunk = (T*)v;
    return OFDM_OK;
  }
  T* at(size_t i) const { return sweep ? sweep + i : chunk; }
};

// a host table of n histogram thresholds into device memory on the launch stream, as kernel arguments: no copy the host waits for
// (ofdm_hest_study.hip)
int study_thresholds_device(const double* thr, size_t n, double* dthr);

}  // namespace ofdm
