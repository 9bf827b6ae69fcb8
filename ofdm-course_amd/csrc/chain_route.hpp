// The route of one Task-5 receiver call (rx_chain_task5_run, ofdm_chain.hip): which entry, front end, estimator kernel, symbol
// stage and DeScrambler placement a plan takes, or why it is refused -- decided once, before anything is launched.  Plain C++
// with no device or runtime dependency: tests/host/chain_route_main.cpp runs it under the host sanitizers against the
// hand-written model of tests/routes.py.  The env switches that select a route are read here, on every call (nothing is cached).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "omp_wide_host.hpp"

namespace ofdm {

constexpr int CH_MAXT = 32;                     // taps of the generic single kernel
constexpr int FAST_MAXT = 32;                   // taps of the fast / split stages
// private LDS of one wavefront's 512-point transform (chain_fast_core.hpp: wave_fft512) and its twiddle tables
constexpr int WAVE_LDS_ELEMS = 512 + 64;
constexpr int WAVE_TW_ELEMS = 2 * 7 * 64;
constexpr int OMP_RT = 8;                       // taps up to which the pursuit's refit is register-resident
constexpr int64_t FAST_MAX_DECISIONS = 48 * 1024;
constexpr size_t GENERIC_LDS_LIMIT = 158 * 1024;
constexpr size_t STAGE_LDS_LIMIT = OMP_STAGE_LDS_LIMIT;   // 150 KiB: the OMP, symbol and eq_demap stages
constexpr size_t SPLIT_LDS_LIMIT = 120 * 1024;
constexpr size_t TWO_WG_LDS_LIMIT = 78 * 1024;            // two workgroups per CU (wave at 8 wavefronts, coop4, r2)
// wave-per-frame symbol stage (ofdm_chain_wave.hip)
constexpr int WV_N = 2048;
constexpr int WV_TR_ELEMS = 576;          // wave-private transpose region (largest index 72*7+63 = 567, 65*7+63 = 518)
constexpr int WV_TW_ROWS = 31;            // W_2048^(lane * kj), kj = 1..31
// dynamic LDS: W_2048 table [31][64] | W_64 table [7][64] | data positions [4][64] (8-byte stride) | per-wave regions
constexpr unsigned WV_OFF_TW = 0, WV_OFF_TWB = 8 * 64 * WV_TW_ROWS, WV_OFF_DD = WV_OFF_TWB + 8 * 64 * 7;
constexpr unsigned WV_OFF_LUT = WV_OFF_DD + 8 * 64 * 4;              // decision thresholds of demap_square_lut
constexpr unsigned WV_OFF_WAVE = WV_OFF_LUT + 256;
constexpr unsigned WV_TRASH_OFF = 8 * WV_TR_ELEMS, WV_DESCR_OFF = WV_TRASH_OFF + 8 * 64, WV_CODES_OFF = WV_DESCR_OFF + 16;
// (WV_DESCR_OFF: one word per wavefront, the DeScrambler state between the pack batches of a frame -- in LDS so that it
//  costs no register across the symbol loop)
// cooperative symbol stage of Nfft 8192 (ofdm_chain_coop.hip)
constexpr int CP_N = 8192, CP_SUB = 2048, CP_R = 4;
constexpr int CP_TR_ELEMS = 576;
constexpr unsigned CP_OFF_TWA = 0, CP_OFF_TWB = 8 * 64 * 7;
constexpr unsigned CP_OFF_WAVE = CP_OFF_TWB + 8 * 64 * 7;
constexpr unsigned CP_OFF_EX = CP_OFF_WAVE + CP_R * 8 * CP_TR_ELEMS;
constexpr unsigned CP_OFF_CODES = CP_OFF_EX + 3 * CP_SUB * 8;

inline size_t route_align16(size_t n) { return (n + 15) & ~size_t(15); }
constexpr int route_fft_lds_elems(int n) { return n + (n >> 3) + 8; }                                  // = fft_lds_elems (fft_core.hpp)
constexpr int route_fft_xforms_per_wg(int n) { return (n / 8 >= 256 ? n / 8 : 256) / (n / 8); }        // = fft_xforms_per_wg

constexpr int route_omp_wave_rs(int taps) { return taps | 1; }                                      // = omp_wave_rs (omp_wave_core.hpp)
// (ofdm_chain.hip holds the static_asserts that tie the three to their originals)

// ---- omp_batch_kernel's dynamic LDS (ofdm_chain_fast.hip)
struct OmpLayout {          // byte offsets into dynamic LDS
  unsigned off_y, off_c0, off_gram, off_state, off_fft, state_bytes, total;
  int fpw;                  // frames per wavefront
  int c0_stride;            // row stride of c0 (k_atoms, or np + 1 when c0 overwrites Y in place)
  int reg_c0;               // wave form with c0 by transform: c0 lands on Y's rows, moves to registers, and the R state takes the bytes
};

inline bool omp_by_fft(int comb_m, int np, int k_atoms) {
  return comb_m == 2048 && np <= 2048 && k_atoms <= 2048 && !std::getenv("OFDM_OMP_NO_FFT");
}

// cs = bytes of one complex element; fft_elems = transform scratch of the by-transform c0 stage, else 0
inline OmpLayout omp_layout(size_t cs, int np, int k_atoms, int taps, int fft_elems) {
  OmpLayout o;
  const bool wave = taps > OMP_RT;            // more than OMP_RT taps: one frame per wavefront (omp_wave_core.hpp)
  // per frame: up to OMP_RT taps nothing (registers); beyond, R = L^-1 [taps][odd stride] complex T
  o.state_bytes = wave ? (unsigned)((cs * (size_t)taps * route_omp_wave_rs(taps) + 15) & ~15u) : 16u;
  const size_t gram_elems = wave ? (size_t)((k_atoms + 511) & ~511) + k_atoms : (size_t)k_atoms;   // two-sided table for the wave form
  const size_t per_frame = cs * (np + 1) + cs * k_atoms + o.state_bytes;
  int fpw = wave ? 1 : 4;     // 16 frames per workgroup: 2 workgroups per CU keep 8 wavefronts in flight
  if (const char* e = std::getenv("OFDM_OMP_FPW")) { const int v = atoi(e); if (!wave && (v == 1 || v == 2 || v == 4 || v == 8)) fpw = v; }
  while (fpw > 1 && 4 * fpw * per_frame + cs * gram_elems > 96 * 1024) fpw >>= 1;
  o.fpw = fpw;
  const int fb = 4 * fpw;
  unsigned b = 0;
  o.c0_stride = k_atoms;
  o.reg_c0 = (wave && fft_elems > 0 && k_atoms <= 512 && k_atoms <= np + 1 && !std::getenv("OFDM_OMP_C0_LDS")) ? 1 : 0;
  const unsigned fft_bytes = (unsigned)((cs * (size_t)fft_elems + 15) & ~15u);
  if (o.reg_c0) {
    // Gram table | { Y rows (c0 written over them) + transform scratch }  ==  { R state of the four frames }: 41.8 KB instead of
    // 74.8 KB at 32 taps, K = Np = 512 -- three resident workgroups per CU instead of two for a pursuit that is bound by the
    // instruction issue of its (few) wavefronts
    o.off_gram = b;  b += (unsigned)((cs * gram_elems + 15) & ~15u);
    o.off_y = b; o.off_c0 = b; o.c0_stride = np + 1;
    const unsigned ybytes = (unsigned)((cs * fb * (np + 1) + 15) & ~15u);
    o.off_fft = b + ybytes;
    o.off_state = b;
    const unsigned st = fb * o.state_bytes;
    b += st > ybytes + fft_bytes ? st : ybytes + fft_bytes;
    o.total = b;
    return o;
  }
  o.off_y = b;     b += (unsigned)((cs * fb * (np + 1) + 15) & ~15u);   // rows padded by one element
  o.off_c0 = b;    b += (unsigned)((cs * fb * k_atoms + 15) & ~15u);
  o.off_gram = b;  b += (unsigned)((cs * gram_elems + 15) & ~15u);
  // the transform scratch of the c0 stage is dead before the per-frame OMP state is first written: same bytes
  o.off_state = b; o.off_fft = b;
  const unsigned st = fb * o.state_bytes;
  b += st > fft_bytes ? st : fft_bytes;
  o.total = b;
  return o;
}

// the layout omp_batch_kernel runs with at a shape, and whether c0 comes from the 2048-point transform
inline OmpLayout omp_batch_layout(bool f64, int comb_m, int np, int k_atoms, int taps, bool* by_fft_out = nullptr) {
  const bool by_fft = omp_by_fft(comb_m, np, k_atoms);
  if (by_fft_out) *by_fft_out = by_fft;
  return omp_layout(f64 ? 16 : 8, np, k_atoms, taps, by_fft ? route_fft_lds_elems(2048) : 0);
}

inline bool omp_mfma_ok(bool f64, int np, int k_atoms) {
  return !f64 && k_atoms % 16 == 0 && np % 4 == 0 && !std::getenv("OFDM_OMP_NO_MFMA");
}

// ---- wave-per-frame symbol stage: the per-wavefront code buffer of a frame
struct WaveLayout {
  unsigned wave_bytes, total;
  int cb;                                 // symbols per pack batch
};

inline bool wave_layout(int nd, int n_symb, int wpb, WaveLayout& lay) {
  // symbols per pack batch: every batch but the last must end on a 32-code boundary
  int cb = 1;
  while ((cb * nd) % 32 != 0) ++cb;                                    // cb <= 32
  const int unit = cb;
  while (cb * nd < 1920 && cb < n_symb) cb += unit;
  if (cb >= n_symb) cb = n_symb;                                       // one batch: the whole frame
  const unsigned codes_bytes = (unsigned)(((size_t)cb * nd + 31 + 32) & ~size_t(31));
  if (codes_bytes > 6144) return false;
  lay.cb = cb;
  lay.wave_bytes = (WV_CODES_OFF + codes_bytes + 15) & ~15u;
  lay.total = WV_OFF_WAVE + (unsigned)wpb * lay.wave_bytes;
  return lay.total <= (wpb == 8 ? 78u : 52u) * 1024;                   // two / three workgroups per CU
}

// eq_demap_kernel's two-carriers-per-lane form (also the Task-4 receiver's, with its own x_stride)
inline bool eq_demap_vec_ok(bool f64, int n_carrier, int x_stride) {
  return !f64 && (n_carrier & 1) == 0 && (x_stride & 1) == 0 && n_carrier <= 2048 && !std::getenv("OFDM_EQD_SCALAR");
}
inline size_t eq_demap_lds_bytes(bool f64, int n_carrier, int64_t decisions) {
  return (size_t)(f64 ? 16 : 8) * n_carrier + (((size_t)decisions + 31) & ~size_t(31)) + 16;
}

// the split form's frame state fits (also asked by the Task-5 part-2 tiles, ofdm_part2.hip)
inline bool chain_split_fits(int taps, int bps, int n_carrier, int64_t decisions, bool f64) {
  if (std::getenv("OFDM_CHAIN_GENERIC")) return false;
  if (taps > FAST_MAXT || bps > 8) return false;
  return (size_t)(f64 ? 16 : 8) * n_carrier + (((size_t)decisions + 31) & ~size_t(31)) <= SPLIT_LDS_LIMIT;
}

// fp32 MMSE mode: H = Sop_banded * (M * Y) instead of the dense operator (asked when the operator is built, and per call)
inline bool mmse_factored_usable(int np, int np_pad) {
  return np % 4 == 0 && np_pad % 16 == 0 && !std::getenv("OFDM_MMSE_NO_MFMA") && !std::getenv("OFDM_MMSE_DENSE");
}

// the factored form in one launch (mmse_fused_kernel) or two (mmse_apply_mfma_kernel<G>, then the banded spline)
inline bool mmse_one_launch(int np_pad) { return np_pad <= 256 && !std::getenv("OFDM_MMSE_TWO_LAUNCHES"); }
// G of mmse_apply_mfma_kernel<G>: 32 rows x 32 frames per wavefront (G = 8 / 4 / 2 / 1 measured: 146 / 129 / 129 / 141 us per 8192 frames)
inline int mmse_factored_g() {
  int g = 4;
  if (const char* e = std::getenv("OFDM_MMSE_G")) g = atoi(e);
  return g >= 8 ? 8 : g >= 4 ? 4 : g >= 2 ? 2 : 1;
}
// the dense operator on the matrix cores (fp32) or mmse_apply_valu_kernel
inline bool mmse_dense_mfma_ok(bool f64, int np, int m_pad) {
  return !f64 && np % 4 == 0 && m_pad % 16 == 0 && !std::getenv("OFDM_MMSE_NO_MFMA");
}

// rx_pilot_omp_kernel: frames per wavefront -- as many as keep the per-group Y / c0 buffer within 8 KB (4 workgroups of ~35 KB per CU)
inline int pilot_omp_fpw(size_t cs, int nw, int ystride) {
  int fpw = 4;
  if (const char* e = std::getenv("OFDM_PILOT_FPW")) { const int v = atoi(e); if (v == 1 || v == 2 || v == 4 || v == 8) fpw = v; }
  while (fpw > 1 && cs * (size_t)nw * fpw * ystride > 8 * 1024) fpw >>= 1;
  return fpw;
}

// ---------------------------------------------------------------------------------------------
enum { EST_OMP = 0, EST_MMSE = 1, EST_MMSE_LS = 2 };                     // ChainShape::estimator

struct ChainShape {
  int nfft, n_symb, n_carrier, np, nd, k_atoms, taps, bps;
  int bits_per_axis;        // 0 unless the constellation is a square QAM (kind == 1)
  int f64;
  int pilots_in_band;
  int comb_m, comb_lg_up, data_mod4;
  int estimator;            // EST_*
  int mmse_factors;         // the fp32 MMSE factors exist (built by ofdm_rx_plan_set_mmse)
  int np_pad, m_pad;
  int descr_on;
  int omp_route;            // OMP_ROUTE_*
  int want_mer;
};

enum { ENTRY_GENERIC, ENTRY_FAST, ENTRY_SPLIT };
enum { FRONT_GENERIC,                   // the generic kernel: everything in one launch
       FRONT_FUSED,                     // rx_pilot_omp_kernel: symbol 1 + OMP in one launch
       FRONT_PILOT,                     // rx_pilot_kernel, then the estimator stage
       FRONT_DEMOD8192_FIRST,           // demod_keep8192 of every frame's first symbol with fused pilot LS (coop4 / r2)
       FRONT_DEMOD8192,                 // demod_keep8192 of all symbols with fused pilot LS, pilot-only rows skipped on data symbols
       FRONT_DEMOD8192_ALL_ROWS,        // the same with every row
       FRONT_DEMOD8192_PLS,             // demod_keep8192 without pilot LS, then pilot_ls_kernel
       FRONT_DEMOD_GENERIC_PLS };       // demod_keep_device, then pilot_ls_kernel
enum { ESTK_IN_KERNEL,                  // generic kernel's own pursuit / the fused launch's (omp_fft)
       ESTK_OMP_FFT, ESTK_OMP_MFMA, ESTK_OMP_SCALAR, ESTK_OMP_WIDE,
       ESTK_MMSE_FUSED, ESTK_MMSE_FACTORED, ESTK_MMSE_DENSE_MFMA, ESTK_MMSE_DENSE_SCALAR, ESTK_MMSE_LS };
enum { SYM_GENERIC, SYM_RX_SYMBOLS, SYM_WAVE, SYM_COOP4, SYM_R2, SYM_EQ_DEMAP };
enum { WAVE_FORM_NONE, WAVE_FORM_SKIP0, WAVE_FORM_SKIP02, WAVE_FORM_EXACT };
enum { DESCR_NONE, DESCR_IN_KERNEL, DESCR_PASS };
enum { ROUTE_OK = 0, REFUSE_OMP_ROUTE, REFUSE_WIDE_GENERIC, REFUSE_MMSE_ENTRY, REFUSE_GENERIC_LDS, REFUSE_OMP_LDS,
       REFUSE_SYMBOL_LDS, REFUSE_EQ_DEMAP_LDS };

struct ChainRoute {
  int entry, front, estimator, symbols, descr;
  int mmse;                 // the symbol stage takes H from the estimator's workspace (HEXT builds)
  int mer, ba;
  // OMP stage
  int omp_taken;            // OMP_ROUTE_BATCH (the fused launch included), OMP_ROUTE_WIDE, 0 = no OMP stage (MMSE modes, generic entry)
  int by_fft, fpw;          // omp_batch_kernel: c0 by the 2048-point transform; frames per wavefront (fused launch: its own)
  OmpLayout omp;            // omp_batch_kernel's layout (estimators ESTK_OMP_FFT / MFMA / SCALAR)
  int mmse_g;               // ESTK_MMSE_FACTORED: mmse_apply_mfma_kernel<G>
  // symbol stage
  int nw, prune;            // SYM_RX_SYMBOLS: rx_symbols_kernel<NW, PRUNE2>; also the front end's rx_pilot(_omp)_kernel
  int wave_form;            // SYM_WAVE
  int vec;                  // SYM_EQ_DEMAP
  size_t generic_lds, symbol_lds;   // bytes of the stages that have a limit (omp.total is the OMP stage's)
};

inline size_t generic_lds_bytes(const ChainShape& s) {    // mirrors chain_layout + launch_chain (ofdm_chain.hip)
  const size_t cs = s.f64 ? 16 : 8;
  size_t b = 0;
  b += route_align16(cs * (size_t)route_fft_lds_elems(s.nfft));
  b += route_align16(cs * (size_t)s.np);
  b += route_align16(cs * (size_t)s.k_atoms);
  b += route_align16(16 * (size_t)CH_MAXT * 2);
  b += route_align16(sizeof(int) * (size_t)(CH_MAXT + 4));
  b += route_align16(16 * (size_t)s.taps * s.taps);
  b += route_align16((size_t)s.nd * s.n_symb);
  return b * (size_t)route_fft_xforms_per_wg(s.nfft);
}

// Returns ROUTE_OK with `r` filled, or a REFUSE_* id with *why = the reason (for REFUSE_OMP_ROUTE the text of omp_route_choose;
// the byte counts the other messages quote are in r.generic_lds / r.omp.total / r.symbol_lds).  When several refusals apply
// the one reported is the first in the order the stages would meet them.
inline int chain_route_choose(const ChainShape& s, ChainRoute& r, const char** why) {
  *why = nullptr;
  r = ChainRoute{};
  const bool f64 = s.f64 != 0, mmse = s.estimator != EST_OMP, mer = s.want_mer != 0, descr = s.descr_on != 0;
  const int64_t decisions = (int64_t)s.nd * s.n_symb;
  r.mmse = mmse; r.mer = mer; r.ba = s.bits_per_axis;
  // ---- entry
  const bool forced_generic = std::getenv("OFDM_CHAIN_GENERIC") != nullptr;
  const bool fast = s.pilots_in_band && !forced_generic && (s.nfft == 512 || s.nfft == 1024 || s.nfft == 2048 || s.nfft == 4096) &&
                    s.taps <= FAST_MAXT && s.bps <= 8 && decisions <= FAST_MAX_DECISIONS;
  r.generic_lds = generic_lds_bytes(s);
  // split form: Nfft beyond the wave-local fast path, a frame state that does not fit the generic kernel's LDS, or MMSE mode
  // outside the fast path
  const bool split = !fast && s.pilots_in_band && chain_split_fits(s.taps, s.bps, s.n_carrier, decisions, f64) &&
                     (s.nfft > 4096 || mmse || r.generic_lds > GENERIC_LDS_LIMIT);
  if (!fast && !split) {
    r.entry = ENTRY_GENERIC; r.front = FRONT_GENERIC; r.estimator = ESTK_IN_KERNEL; r.symbols = SYM_GENERIC;
    r.descr = descr ? DESCR_PASS : DESCR_NONE;
    if (mmse) { *why = "the MMSE mode of a plan needs the fast or the split form"; return REFUSE_MMSE_ENTRY; }
    if (s.omp_route == OMP_ROUTE_WIDE) { *why = "the wide OMP route needs the three-launch receiver"; return REFUSE_WIDE_GENERIC; }
    if (r.generic_lds > GENERIC_LDS_LIMIT) { *why = "the generic kernel's LDS"; return REFUSE_GENERIC_LDS; }
    return ROUTE_OK;
  }
  r.entry = fast ? ENTRY_FAST : ENTRY_SPLIT;
  r.nw = s.nfft / 512;
  r.prune = s.n_carrier <= 128 * r.nw;
  // ---- estimator
  bool by_fft = false;
  if (!mmse) {
    r.omp = omp_batch_layout(f64, s.comb_m, s.np, s.k_atoms, s.taps, &by_fft);
    r.omp_taken = OMP_ROUTE_BATCH;
    if (s.omp_route != OMP_ROUTE_BATCH) {        // AUTO / WIDE: a shape the chosen kernel cannot serve is refused before any launch
      r.omp_taken = omp_route_choose(s.omp_route, r.omp.total, s.nfft, s.k_atoms, s.taps, why);
      if (!r.omp_taken) { r.omp_taken = OMP_ROUTE_BATCH; return REFUSE_OMP_ROUTE; }
    }
    r.by_fft = by_fft; r.fpw = r.omp.fpw;
    r.estimator = r.omp_taken == OMP_ROUTE_WIDE ? ESTK_OMP_WIDE : by_fft ? ESTK_OMP_FFT
                  : omp_mfma_ok(f64, s.np, s.k_atoms) ? ESTK_OMP_MFMA : ESTK_OMP_SCALAR;
  } else if (s.estimator == EST_MMSE_LS) {
    r.estimator = ESTK_MMSE_LS;
  } else if (!f64 && s.mmse_factors && mmse_factored_usable(s.np, s.np_pad)) {
    if (mmse_one_launch(s.np_pad)) r.estimator = ESTK_MMSE_FUSED;
    else { r.estimator = ESTK_MMSE_FACTORED; r.mmse_g = mmse_factored_g(); }
  } else {
    r.estimator = mmse_dense_mfma_ok(f64, s.np, s.m_pad) ? ESTK_MMSE_DENSE_MFMA : ESTK_MMSE_DENSE_SCALAR;
  }
  const bool omp_lds_over = !mmse && r.omp_taken == OMP_ROUTE_BATCH && r.omp.total > STAGE_LDS_LIMIT;
  if (fast) {
    const bool fused = !mmse && s.comb_lg_up >= 0 && s.taps <= OMP_RT && s.k_atoms <= 512 && s.omp_route != OMP_ROUTE_WIDE &&
                       !std::getenv("OFDM_FAST_UNFUSED");
    if (fused) {
      // kernels 1+2 in one launch (comb pilots): c0 by a wave-local inverse transform (ofdm_chain_pilot.hip)
      r.front = FRONT_FUSED; r.estimator = ESTK_IN_KERNEL; r.omp_taken = OMP_ROUTE_BATCH; r.by_fft = 1;
      r.fpw = pilot_omp_fpw(f64 ? 16 : 8, r.nw, s.np > s.k_atoms ? s.np : s.k_atoms);
    } else {
      r.front = FRONT_PILOT;
      if (omp_lds_over) { *why = "the OMP stage's LDS"; return REFUSE_OMP_LDS; }
    }
    // one wavefront per frame (ofdm_chain_wave.hip) whenever its conditions hold, DeScrambler or not; a MER request under the
    // exact-slicer switch takes the four-wavefront MER variant
    WaveLayout wl;
    const bool exact = std::getenv("OFDM_WAVE_EXACT_SLICER") != nullptr;
    const bool wave = !f64 && s.nfft == WV_N && s.n_carrier <= WV_N / 4 && s.taps <= FAST_MAXT && !std::getenv("OFDM_FAST_NO_WAVE") &&
                      wave_layout(s.nd, s.n_symb, 4, wl) && wave_layout(s.nd, s.n_symb, 8, wl) && !(mer && exact);
    if (wave) {
      r.symbols = SYM_WAVE;
      // no data carrier with index = 0 (mod 4) -- pilots "1:4:end", the benchmark layout: the round of that residue class is not
      // computed on data symbols; pilots 1:2:end: two of the four rounds
      const bool no_skip = std::getenv("OFDM_WAVE_NO_SKIP") != nullptr;
      r.wave_form = exact ? WAVE_FORM_EXACT : ((s.data_mod4 & 15) == 14 && !no_skip) ? WAVE_FORM_SKIP0
                    : ((s.data_mod4 & 15) == 10 && !no_skip) ? WAVE_FORM_SKIP02 : WAVE_FORM_NONE;
    } else {
      r.symbols = SYM_RX_SYMBOLS;
      r.symbol_lds = (size_t)(f64 ? 16 : 8) * ((size_t)r.nw * WAVE_LDS_ELEMS + WAVE_TW_ELEMS) + (((size_t)decisions + 31) & ~size_t(31));
      if (r.symbol_lds > STAGE_LDS_LIMIT) { *why = "the symbol stage's LDS"; return REFUSE_SYMBOL_LDS; }
    }
    // DeScrambler: in the pack stage of the wave kernel, which has such builds in OMP mode without MER only; else the pass
    r.descr = !descr ? DESCR_NONE : (wave && !mer && !mmse) ? DESCR_IN_KERNEL : DESCR_PASS;
    return ROUTE_OK;
  }
  // ---- split form
  r.descr = descr ? DESCR_PASS : DESCR_NONE;
  if (omp_lds_over) { *why = "the OMP stage's LDS"; return REFUSE_OMP_LDS; }
  if (!f64) {
    // coop4: Nfft 8192, N_carrier <= 2048, K <= 512, no data carrier on the residue class 0 (mod 4), whole 32-code groups per
    // symbol (the faster one where its layout conditions hold); r2 otherwise.  Neither descrambles: a DeScrambler plan hands the
    // raw decisions of either to descr_pass_kernel
    const bool coop = !std::getenv("OFDM_SPLIT_NO_COOP") && s.nfft == CP_N && s.n_carrier <= CP_N / 4 && s.k_atoms <= 512 &&
                      s.taps <= FAST_MAXT && (s.data_mod4 & 1) == 0 && (s.nd & 31) == 0 && s.n_symb >= 1 &&
                      CP_OFF_CODES + 2u * (unsigned)((s.nd + 63) & ~31) <= TWO_WG_LDS_LIMIT;
    const size_t r2_lds = 8 * ((size_t)8 * WAVE_LDS_ELEMS + WAVE_TW_ELEMS) + (((size_t)decisions + 31) & ~size_t(31));
    const bool r2 = !coop && !std::getenv("OFDM_SPLIT_NO_R2") && s.nfft == 8192 && s.n_carrier <= 2048 && s.taps <= FAST_MAXT &&
                    s.n_symb >= 1 && r2_lds <= TWO_WG_LDS_LIMIT;
    if (coop || r2) {
      r.front = FRONT_DEMOD8192_FIRST;
      r.symbols = coop ? SYM_COOP4 : SYM_R2;
      r.symbol_lds = coop ? CP_OFF_CODES + 2u * (unsigned)((s.nd + 63) & ~31) : r2_lds;
      return ROUTE_OK;
    }
  }
  if (s.nfft == 8192 && !std::getenv("OFDM_SPLIT_GENERIC_FFT")) {
    // the pilot LS values come out of the transform of each frame's first symbol (no pilot_ls pass); the rows of pilot-only
    // sub-transforms are skipped on data symbols -- only when the pilot LS values come out of this kernel
    r.front = std::getenv("OFDM_SPLIT_NO_PLS_FUSE") ? FRONT_DEMOD8192_PLS
              : std::getenv("OFDM_SPLIT_ALL_ROWS") ? FRONT_DEMOD8192_ALL_ROWS : FRONT_DEMOD8192;
  } else {
    r.front = FRONT_DEMOD_GENERIC_PLS;
  }
  r.symbols = SYM_EQ_DEMAP;
  r.vec = eq_demap_vec_ok(f64, s.n_carrier, s.n_carrier);
  r.symbol_lds = eq_demap_lds_bytes(f64, s.n_carrier, decisions);
  if (r.symbol_lds > STAGE_LDS_LIMIT) { *why = "the equalise / demap stage's LDS"; return REFUSE_EQ_DEMAP_LDS; }
  return ROUTE_OK;
}

}  // namespace ofdm
