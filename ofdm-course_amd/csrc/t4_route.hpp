// The route of one Task-4 receiver call (task4_run, ofdm_chain_t4.hip): which kernels the autocorrelation, IFO, demodulator,
// fine-sync / estimate and channel stages take, or why the call is refused -- decided once, before anything is launched or
// allocated.  Plain C++ with no device or runtime dependency: tests/host/t4_route_main.cpp runs it under the host sanitizers
// against the hand-written model of tests/t4_routes.py.  The five OFDM_T4_* switches that select a route are read here, on every
// call (nothing is cached).  A refused call used to leave the launches of the stages before the refusal behind (device-resident
// outputs written, nothing returned to host callers); now it leaves none.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "chain_route.hpp"      // eq_demap_vec_ok

namespace ofdm {

constexpr int T4_ACF_MAXW = 1024;                 // = ACF_MAXW (sync_core.hpp), the "1024" of the first refusal's text
constexpr int T4_WAVE_NFFT = 2048;                // = T4W_N, the wave demodulator's Nfft (ofdm_t4_wave.hip)
constexpr size_t T4_FINE_EST_LDS_LIMIT = 48 * 1024;

struct T4Shape {            // what task4_run reads from the plan and its arguments
  int nfft, t_guard, n_symb, n_carrier, np, f64;
  int time_desync, freq_desync, mp_desync;
  int band_tables;          // the plan has the spline operator's fp32 band (t4_plan_tables builds it on every fp32 plan)
};

enum { T4_ACF_NONE, T4_ACF_SEARCH,          // t4_acf_search_kernel: one launch, no curve in HBM
       T4_ACF_FULL };                       // acf_kernel + acf_plateau_kernel + t4_scalars_kernel (OFDM_T4_FULL_ACF)
enum { T4_FORM_DIRECT,                      // no aligned copy of the batch: the IFO search and the demodulator read rx
       T4_FORM_STAGED };                    // t4_align_kernel first; the stages work on the aligned stream and the full grid
enum { T4_IFO_NONE, T4_IFO_WAVE,            // t4_ifo_wave_kernel
       T4_IFO_SEGMENT_DIRECT,               // t4_segment_direct_kernel + transform + first_above_kernel + t4_ifo_finalize_kernel
       T4_IFO_SEGMENT_STAGED };             // t4_segment_kernel + transform + first_above_kernel + t4_ifo_kernel
enum { T4_DEMOD_WAVE,                       // t4_demod_wave_kernel
       T4_DEMOD_NW,                         // t4_demod_kernel<T, nw>
       T4_DEMOD_DEVICE };                   // demod_device on the aligned stream
enum { T4_EST_NONE, T4_EST_FUSED,           // t4_fine_est_kernel
       T4_EST_TAU_PHASE,                    // fine_tau_kernel + fine_phase_kernel; the rotation is applied where X is read
       T4_EST_TAU_PHASE_APPLY };            // the same + fine_apply_kernel over X (staged form)
enum { T4_MEANS_NONE, T4_MEANS_FUSED,       // in t4_fine_est_kernel
       T4_MEANS_KERNEL };                   // t4_mean_pilots_kernel
enum { T4_CH_ONES,                          // t4_fill_ones_kernel
       T4_CH_BAND,                          // spline_band_kernel (which hands a band beyond its LDS back to the dense product)
       T4_CH_DENSE };                       // t4_apply_operator_kernel
enum { T4_ROUTE_OK = 0, T4_REFUSE_GUARD, T4_REFUSE_IFO_SEGMENT, T4_REFUSE_PILOTS };

struct T4Route {
  int acf, form, ifo, demod, est, means, channel;
  int nw;                   // T4_DEMOD_NW: 1, 2, 4 or 8
  int sync;                 // time_desync or freq_desync
  // derived once for the launches
  int pilots_compact;       // the pilot rows are read from the demodulator's compact [np x n_symb] copy, not from the full grid
  int64_t pilot_fstride;    // elements between the frames of that source
  int lazy_rot;             // fine_sync's rotation is applied where X is read (pilot means, equaliser), X is not rewritten
  int x_stride;             // rows of X per symbol as the equaliser reads it
  int eq_vec;               // eq_demap_kernel's two-carriers-per-lane form
  size_t fine_est_lds;      // T4_EST_FUSED: dynamic LDS of t4_fine_est_kernel
};

inline bool t4_demod_wave_supported(int nfft, int n_keep, bool f64) {
  return !f64 && nfft == T4_WAVE_NFFT && n_keep <= 1024 && (n_keep & 1) == 0 && !std::getenv("OFDM_T4_NO_WAVE");   // even: 16-byte row alignment
}

// Returns T4_ROUTE_OK with `r` filled, or a T4_REFUSE_* id with *why = the message.  The refusals are met in the order of the
// stages that used to raise them (the second cannot be met behind the first: a frame of two symbols holds 2 * Nfft samples).
inline int t4_route_choose(const T4Shape& s, T4Route& r, const char** why) {
  *why = nullptr;
  r = T4Route{};
  const bool f64 = s.f64 != 0, sync = s.time_desync || s.freq_desync;
  const int N = s.nfft;
  const int64_t len = (int64_t)(N + s.t_guard) * s.n_symb, n_out = len - s.t_guard - N;
  r.sync = sync;
  if (sync && !(n_out > 0 && s.t_guard >= 1 && s.t_guard <= T4_ACF_MAXW)) {
    *why = "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024";
    return T4_REFUSE_GUARD;
  }
  if (s.freq_desync && len < 2 * (int64_t)N) { *why = "rx_chain_task4: rx_signal(Nfft+1:2*Nfft) exceeds the frame"; return T4_REFUSE_IFO_SEGMENT; }
  if (sync && s.np < 2) { *why = "rx_chain_task4: fine_sync needs at least two pilot carriers"; return T4_REFUSE_PILOTS; }
  const bool full_acf = std::getenv("OFDM_T4_FULL_ACF") != nullptr;       // the curve in HBM + the search over it (A/B, tests)
  r.acf = !sync ? T4_ACF_NONE : full_acf ? T4_ACF_FULL : T4_ACF_SEARCH;
  const bool direct = (N == 512 || N == 1024 || N == 2048 || N == 4096) && !std::getenv("OFDM_T4_STAGED");
  r.form = direct ? T4_FORM_DIRECT : T4_FORM_STAGED;
  // Nfft 2048, fp32, N_carrier <= 1024: one wavefront per symbol run, and segment, spectrum and search of remove_IFO.m:5-8 in one launch
  const bool wave = direct && t4_demod_wave_supported(N, s.n_carrier, f64);
  r.ifo = !s.freq_desync ? T4_IFO_NONE : wave ? T4_IFO_WAVE : direct ? T4_IFO_SEGMENT_DIRECT : T4_IFO_SEGMENT_STAGED;
  r.demod = wave ? T4_DEMOD_WAVE : direct ? T4_DEMOD_NW : T4_DEMOD_DEVICE;
  r.nw = r.demod == T4_DEMOD_NW ? N / 512 : 0;
  // direct form: fine_sync's two estimates and the pilot means in ONE launch on the frame's compact pilot rows held in LDS
  r.fine_est_lds = 16 * (size_t)s.np;
  const bool fused = direct && r.fine_est_lds <= T4_FINE_EST_LDS_LIMIT && (sync || s.mp_desync) && !std::getenv("OFDM_T4_UNFUSED_SYNC");
  r.est = fused ? T4_EST_FUSED : !sync ? T4_EST_NONE : direct ? T4_EST_TAU_PHASE : T4_EST_TAU_PHASE_APPLY;
  r.means = !s.mp_desync ? T4_MEANS_NONE : fused ? T4_MEANS_FUSED : T4_MEANS_KERNEL;
  // fp32: banded product (0.084 -> 0.04 ms per 4096 frames at C3), else the dense tile product
  r.channel = !s.mp_desync ? T4_CH_ONES : (!f64 && s.band_tables && !std::getenv("OFDM_T4_DENSE_SPLINE")) ? T4_CH_BAND : T4_CH_DENSE;
  r.pilots_compact = direct;
  r.pilot_fstride = direct ? (int64_t)s.np * s.n_symb : (int64_t)N * s.n_symb;
  r.lazy_rot = sync && direct;
  r.x_stride = direct ? s.n_carrier : N;
  r.eq_vec = eq_demap_vec_ok(f64, s.n_carrier, r.x_stride);
  return T4_ROUTE_OK;
}

// ---- the plan arena (pl->ws_t4) of one call over F frames: byte offsets of its regions, each padded to 256 bytes
struct T4Arena {
  size_t res, resv, y, X, est, hp, H, Xp, rho, seg, spec, first, total;
};
constexpr int T4_ARENA_REGIONS = 12;

inline T4Arena t4_arena_layout(const T4Shape& s, const T4Route& r, int64_t F) {
  T4Arena a{};
  const size_t cs = s.f64 ? 16 : 8, N = (size_t)s.nfft, S = (size_t)s.n_symb, np = (size_t)s.np, nf = (size_t)F;
  const size_t len = (N + s.t_guard) * S;
  auto reserve = [&](size_t bytes) { const size_t o = a.total; a.total += (bytes + 255) & ~size_t(255); return o; };
  a.res = reserve(sizeof(int64_t) * 2 * nf);         // acf_plateau_kernel's result (T4_ACF_FULL)
  a.resv = reserve(sizeof(double) * 2 * nf);
  a.y = reserve(cs * len * nf);                      // the aligned stream (staged form)
  a.X = reserve(cs * N * S * nf);                    // the demodulated symbols
  a.est = reserve(sizeof(double) * 2 * nf);          // fine_sync's tau and phase
  a.hp = reserve(cs * np * nf);                      // the pilot means
  a.H = reserve(cs * (size_t)s.n_carrier * nf);
  a.Xp = reserve(cs * np * S * nf);                  // the compact pilot rows (direct form)
  a.rho = reserve(r.acf == T4_ACF_FULL ? cs * (len - s.t_guard - N) * nf : 0);
  a.seg = reserve(s.freq_desync ? cs * N * nf : 0);  // remove_IFO's segment, its spectrum and the first line above the threshold
  a.spec = reserve(s.freq_desync ? cs * N * nf : 0);
  a.first = reserve(s.freq_desync ? sizeof(int64_t) * nf : 0);
  return a;
}

// bytes per frame of that arena as the BER sweep budgets its chunks (txf_chunk_task4, txf_plan.hpp), the rho region of OFDM_T4_FULL_ACF not
// counted: the regions above (+ the per-frame scalars) and the frame's packed bits
inline size_t t4_frame_bytes(const T4Shape& s, int frame_words) {
  const size_t cs = s.f64 ? 16 : 8;
  const size_t len = (size_t)(s.nfft + s.t_guard) * s.n_symb;
  return cs * (len + (size_t)s.nfft * s.n_symb + (size_t)s.np * s.n_symb + 2 * (size_t)s.nfft + s.np +
               s.n_carrier) + 128 + (size_t)frame_words * 4;
}

}  // namespace ofdm
