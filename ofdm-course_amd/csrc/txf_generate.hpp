// What the BER sweeps (ofdm_ber_sweep.hip) use of the fused frame generator (ofdm_txfused.hip): the chunk buffers carved from
// the plan-owned workspace and the generation of one chunk into them.  The decisions of a call are txf_plan.hpp's.
#pragma once

#include "channel_resp.hpp"
#include "rx_plan.hpp"
#include "txf_plan.hpp"

namespace ofdm {

static_assert(TXF_DESCR_ON == DESCR_ON, "txf_plan.hpp restates DESCR_ON");

int tx_dict_device(ofdm_rx_plan* pl);                // ofdm_txgen.hip

// the Task-4 impairments of a generator call (T4/Main_model_Task_4.m:99-110): modes 0 off, 1 fixed, 2 drawn; the chunk's
// per-frame draws are written to sto / cfo (nf entries each)
struct TxfImp {
  int sto_mode = 0;
  int64_t sto_value = 0;
  int cfo_mode = 0;
  double cfo_value = 0;
  int64_t* sto = nullptr;
  double* cfo = nullptr;
  TxfImp() = default;
  TxfImp(int sm, int64_t sv, int cm, double cv) : sto_mode(sm), sto_value(sv), cfo_mode(cm), cfo_value(cv) {}
};

// a per-frame channel on the delay line of a TxfChannel (txf_fading), the amplitudes drawn per chunk
struct TxfFade {
  TxfGains gains;
  c64* amp = nullptr;                                // the chunk's amplitudes [nf][n_taps] (tx_fade_draw_kernel)
  c64* taps_out = nullptr;                           // generator: where the caller wants them (optional)
};

// chunk buffers inside the plan-owned workspace, one per region of txf_plan.hpp's table (null: the call has no such region)
struct TxfBuffers {
  void* tx = nullptr;
  double* partial = nullptr;
  uint8_t *b0 = nullptr, *b1 = nullptr;
  void* rx = nullptr;
  uint32_t* ref = nullptr;
  int64_t* sto = nullptr;
  double* cfo = nullptr;
  c64* amp = nullptr;
  void* hest = nullptr;
};

// the bit source of a chunk where it is not the Philox draw: the caller's packed stream (ofdm_payload.hip), staged as words with a
// zero word behind it; the chunk's first frame is frame `frame` of the call (payload_position, payload_plan.hpp)
struct TxfPayload {
  const uint32_t* words = nullptr;
  int64_t n_bits = 0, first_frame = 0, period = INT64_MAX;
  int64_t frame = 0;                                 // set per chunk by the loop that generates it
};

// payload_frames_kernel: the chunk's bits, one byte each (b0: what ofdm_Scrambler_frames and txf_symbols read), and its packed
// reference words (ref, optional)
int payload_frames_device(const ofdm_rx_plan* pl, const TxfPayload& src, int64_t nf, uint8_t* b0, uint32_t* ref);
// the caller's packed stream of n_bits (where the call's flags say) as words in device memory with a zero word behind it
int payload_stage(Stage& st, const uint8_t* payload, int64_t n_bits, const uint32_t** words);

// what the checks of txf_plan.hpp read from a plan, and a refusal of theirs as the entry's return code and last-error text
TxfShape txf_shape(const ofdm_rx_plan* pl);
int txf_refused(int id, const TxfWhy& w);

// grows pl->ws_txf to txf_layout(ch frames) and carves b from it
int txf_workspace(ofdm_rx_plan* pl, int64_t ch, const TxfUse& u, TxfBuffers& b);

// the symbol stage alone (tx_symbols_fused_kernel): the TX samples of nf frames and their per-symbol sums |x|^2; sc_bits: the
// frames' bits, one byte each, in place of the Philox payload (null: the payload draw).  The PAPR study's stage 1.
int txf_symbols(const ofdm_rx_plan* pl, void* tx, double* partial, const uint8_t* sc_bits, uint32_t k0, uint32_t k1,
                uint32_t stream0, int64_t nf);

// one chunk of nf frames (streams stream0 ..): rx, the packed payload bits (ref) and the packed scrambled bits (scref)
// imp (optional): the Task-4 impairments, the channel pass of tx_channel_imp_kernel
// fade (optional): a channel per frame -- the draws into fade->amp (and fade->taps_out), the channel pass of
// tx_channel_fade_kernel; with imp too, both draws and the channel pass of tx_channel_imp_fade_kernel
// src (optional): the frames' bits from the caller's stream in place of the payload draw (b.b0 is then needed even without the
// Scrambler); every other draw of frame f stays that of Philox stream stream0 + f
int txf_generate(ofdm_rx_plan* pl, const TxfChannel& ch, double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0, int64_t nf,
                 const uint8_t* scr_reg15, const TxfBuffers& b, void* rx, uint32_t* ref, uint32_t* scref,
                 const TxfImp* imp = nullptr, const TxfFade* fade = nullptr, const TxfPayload* src = nullptr);

// ofdm_ber_sweep.hip, for the channel study beside the Task-4 sweep: the channel-estimate error sum_k |H_f(k) - hest[f][k]|^2 of
// nf frames (t5_frame_nmse_kernel; amp_stride: dl.n for a channel per frame, 0 for one static channel), the delays of a call's
// channel, the taps of a static channel into device memory, and the fixed-order sum of one double per frame over every point
int txf_frame_nmse(const ofdm_rx_plan* pl, const c64* amp, const void* hest, const TxfDelays& dl, int64_t amp_stride, int64_t nf,
                   double* frame_nmse);
TxfDelays txf_delays(const TxfChannel& ch);
int txf_static_amps(const TxfChannel& ch, c64* damp);
int txf_point_sums1(const void* frame_values, int64_t n_points, int64_t frames_per_point, void* sums);

}  // namespace ofdm
