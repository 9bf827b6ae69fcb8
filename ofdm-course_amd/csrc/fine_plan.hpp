// The plan of one call of the fine-sync capture (ofdm_fine_study.hip): ofdm_rx_fine, the per-pilot-pair residual-delay curve `taus`
// of fine_sync (T4/fine_sync.m:10-30, T5/fine_sync.m:8-16; figures 18a / 18b of the Task-4 report) with its mask (:33 / T5 :18), the
// two estimates and their denominators for a batch of the caller's demodulated frames, and ofdm_fine_study, those curves summed
// over the frames of every point of a sweep of the fused generator behind the front end of the Task-4 receiver, with the histogram
// of the timing error (T4/Main_model_Task_4.m:137-203).  The argument checks of both entries in the order they are made, the
// length of `taus`, the chunk the generator's workspace, the receiver's arena and the chunk's rows allow, the launch shape of the
// two kernels, and the two small functions every layer shares: the timing error of a frame and the bin it falls into.  Plain C++
// with no device or runtime dependency (FINE_HD is empty outside a device compile): tests/host/fine_plan_main.cpp runs it under
// the host sanitizers against tests/fine_cases.py.  The .hip side turns a refusal into OFDM_ERR_ARG (TXF_REFUSE_DEVICE:
// OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sync_plan.hpp"     // sync_phase_bin, SYNC_LDS_LIMIT; txf_plan.hpp and t4_route.hpp through it

#if defined(__HIPCC__)
#define FINE_HD __host__ __device__
#else
#define FINE_HD
#endif

namespace ofdm {

// sync_core.hpp's FS_THREADS / FS_U and the bytes of its FsScratch, restated (ofdm_fine_study.hip asserts them)
constexpr int FINE_THREADS = 256;
constexpr int FINE_U = 4;
constexpr size_t FINE_SCRATCH_BYTES = 88;

enum { FINE_VARIANT_T5 = 0, FINE_VARIANT_T4 = 1 };   // the `variant` of ofdm_fine_sync

// the refusals of the two entries: a TXF_REFUSE_* of txf_plan.hpp, or one of their own
enum { FINE_REFUSE_FRAMES = TXF_REFUSALS, FINE_REFUSE_BOTH, FINE_REFUSE_VARIANT, FINE_REFUSE_PILOTS, FINE_REFUSE_LONG, FINE_REFUSE_SYNC,
       FINE_REFUSE_ROUTE, FINE_REFUSE_BINS, FINE_REFUSE_OUTPUT, FINE_REFUSALS };

// ---- the length of `taus`: T5/fine_sync.m:8 allocates numel(pilotValues) = Np * N_symb entries and its loop leaves the last one
// 0; T4/fine_sync.m:8 allocates Np and lets the loop of :25-30 grow it to numel - 1 entries -- no trailing 0 -- unless numel - 1 < Np
// (one symbol), where the Np allocated entries stay.  What fine_tau_body walks.
inline int64_t fine_len(int64_t np, int64_t n_symb, int variant) {
  const int64_t M = np * n_symb;
  return (variant == FINE_VARIANT_T4 && M - 1 >= np) ? M - 1 : M;
}

// ---- the histogram of the timing error: n bins of equal width on [lo, hi)
struct FineBins {
  int n = 0;
  double lo = 0.0, hi = 0.0;
};

enum { FINE_BIN_BELOW = -1, FINE_BIN_ABOVE = -2, FINE_BIN_NAN = -3 };

// The bin of e: FINE_BIN_NAN for a value that is not finite (tau = mean([]) = NaN), FINE_BIN_BELOW for e < lo, FINE_BIN_ABOVE for
// e >= hi, else floor((e - lo) * n / (hi - lo)), held to n - 1 where the quotient rounds up to n.  A difference, a product and a
// quotient: nothing a compiler can contract, so every layer gets the same bin.
FINE_HD inline int fine_bin(double e, int n, double lo, double hi) {
  if (!(e - e == 0.0)) return FINE_BIN_NAN;
  if (e < lo) return FINE_BIN_BELOW;
  if (!(e < hi)) return FINE_BIN_ABOVE;
  const double q = (e - lo) * (double)n / (hi - lo);
  const int b = (int)q;
  return b < n ? b : n - 1;
}

// The timing error of a frame in samples: e = tau * Nfft + phi_s + 1, phi = sync_phase_bin(TgPosition, Time_Delay, Nfft + T_guard)
// the guard phase the coarse synchroniser left the frame at, phi_s = phi wrapped into (-(Nfft + T_guard) / 2, (Nfft + T_guard) / 2].
// The window of T4/Main_model_Task_4.m:292-294 at phi_s = 0 is one sample late (tau * Nfft = -1 on a clean frame), and every sample
// it is early adds one to tau * Nfft: e is 0 where fine_sync measures what the coarse stage left.  Nfft is a power of two, so the
// product is exact and a fused multiply-add gives the same double as a product and a sum.  NaN for tau = NaN.
FINE_HD inline double fine_tau_err(double tau, int64_t tg_position, int64_t time_delay, int nfft, int64_t stride) {
  const int64_t phi = sync_phase_bin(tg_position, time_delay, stride);
  const int64_t phi_s = phi > stride - phi ? phi - stride : phi;       // 2 phi > stride, without the doubling
  return tau * (double)nfft + (double)(phi_s + 1);
}

// ---- the capture of one call
struct FineCapture {
  int variant = FINE_VARIANT_T4;
  bool out = false;          // an output is given
};

// The capture checks, in this order: variant T4 / T5 -> at least two pilots (deltak of fine_sync.m:6 needs two) -> Np * N_symb <
// 2^31 (the kernels index a frame's pilots in 32 bits)
inline int fine_check_capture(const TxfShape& s, const FineCapture& c, const char* what, TxfWhy& w) {
  if (!(c.variant == FINE_VARIANT_T4 || c.variant == FINE_VARIANT_T5))
    return txf_refuse(w, FINE_REFUSE_VARIANT, "%s: variant must be 0 (T5/fine_sync.m) or 1 (T4/fine_sync.m) (%d)", what, c.variant);
  if (!(s.np >= 2)) return txf_refuse(w, FINE_REFUSE_PILOTS, "%s: fine_sync needs at least two pilot carriers (%d)", what, s.np);
  if (!((int64_t)s.np * s.n_symb < ((int64_t)1 << 31)))
    return txf_refuse(w, FINE_REFUSE_LONG, "%s: Np * N_symb must be below 2^31 (%lld)", what, (long long)((int64_t)s.np * s.n_symb));
  return TXF_OK;
}

// ---- ofdm_rx_fine.  The order of its checks; the first that fails is the refusal a caller sees.
//   bad arguments (plan, X) -> the plan as txf_check_plan reads it (device, precision, data carriers, pilots in band,
//   Nfft / T_guard) -> n_frames 0 .. 2^31 - 1 -> the capture (above) -> an output is given
inline int fine_rx_prelude(const TxfShape* plan, bool x, bool f64_flag, int64_t n_frames, const FineCapture& cap, TxfWhy& w) {
  static const char* const WHAT = "rx_fine";
  if (const int id = txf_check_args(plan && x, WHAT, w)) return id;
  if (const int id = txf_check_plan(*plan, f64_flag, 0, 0, WHAT, w)) return id;
  if (!(n_frames >= 0 && n_frames < ((int64_t)1 << 31)))
    return txf_refuse(w, FINE_REFUSE_FRAMES, "%s: n_frames must be 0 .. 2^31 - 1 (%lld)", WHAT, (long long)n_frames);
  if (const int id = fine_check_capture(*plan, cap, WHAT, w)) return id;
  if (!cap.out) return txf_refuse(w, FINE_REFUSE_OUTPUT, "%s: no output is given", WHAT);
  return TXF_OK;
}

// ---- ofdm_fine_study.  The order of its checks: the front every study shares (txf_study_prelude: the generator's arguments,
// max_frames_per_chunk 0 .. 65535, the receiver's limit) -> the capture (above) -> both sync flags off -> the route of the
// receiver's front end (t4_route_choose, in the receiver's words) -> the bins (n >= 1, lo < hi, both finite) -> an output
inline int fine_study_prelude(const TxfCall& c, bool both_channels, int time_desync, int freq_desync, const FineCapture& cap,
                              const FineBins& bins, TxfChannel& ch, TxfGains& g, TxfWhy& w) {
  static const char* const WHAT = "fine_study";
  if (const int id = txf_study_prelude(c, both_channels, FINE_REFUSE_BOTH, WHAT, ch, g, w, 65535)) return id;
  if (const int id = fine_check_capture(*c.plan, cap, WHAT, w)) return id;
  if (!(time_desync || freq_desync))
    return txf_refuse(w, FINE_REFUSE_SYNC, "%s: time_desync and freq_desync are both off: the receiver runs no fine_sync, there is nothing to study", WHAT);
  const TxfShape& s = *c.plan;
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, time_desync ? 1 : 0, freq_desync ? 1 : 0, 0, 0};
  T4Route r;
  const char* why = nullptr;
  if (t4_route_choose(t4, r, &why) != T4_ROUTE_OK) return txf_refuse(w, FINE_REFUSE_ROUTE, "%s: %s", WHAT, why);
  if (!(bins.n >= 1 && bins.lo < bins.hi && bins.lo - bins.lo == 0.0 && bins.hi - bins.hi == 0.0))
    return txf_refuse(w, FINE_REFUSE_BINS, "%s: bins must have n >= 1 and finite lo < hi (%d, %g, %g)", WHAT, bins.n, bins.lo, bins.hi);
  if (!cap.out) return txf_refuse(w, FINE_REFUSE_OUTPUT, "%s: no output is given", WHAT);
  return TXF_OK;
}

// ---- the chunk of the study: frames of one point, budgeted as the Task-4 sweep budgets its chunks (the generator's regions with
// the RX region and the receiver's arena, on twice the workspace budget) and, beside them, per frame one row of L doubles (`taus`),
// L bytes of mask, and the frame's scalars (tau, phase, the timing error, TgPosition, FreqOffset, the Time_Delay copy: 8 bytes
// each; n_used, n_phase, IFO, status: 4 each).
constexpr size_t FINE_SCALAR_BYTES = 64;

inline size_t fine_row_bytes(const TxfShape& s, int variant) {
  return (sizeof(double) + 1) * (size_t)fine_len(s.np, s.n_symb, variant) + FINE_SCALAR_BYTES;
}

inline int64_t fine_chunk(const TxfShape& s, const TxfUse& u, int64_t frames_per_point, int64_t user_cap, int variant,
                          size_t budget = 2 * TXF_WS_BUDGET) {
  const T4Shape t4{s.nfft, s.t_guard, s.n_symb, s.n_carrier, s.np, s.f64, 0, 0, 0, 0};
  return txf_chunk(s, u, frames_per_point, user_cap, budget, t4_frame_bytes(t4, s.frame_words) + fine_row_bytes(s, variant));
}

// ---- the launch shape.  fine_capture_kernel: one workgroup of FINE_THREADS threads per frame, the static LDS of the two
// reductions only (the rows are written as they are formed).  fine_accumulate_kernel: the studies' accumulate launch
// (txf_plan.hpp: STUDY_ACC_*) over the L entries of the curve, with the tail workgroup for the chunk's per-frame scalars.
static_assert(FINE_SCRATCH_BYTES <= SYNC_LDS_LIMIT, "the capture kernel's LDS");

struct FinePass {
  int threads;               // FINE_THREADS
  unsigned grid;             // frames: one workgroup each
  size_t lds;                // static LDS of the capture kernel
  int trips;                 // ceil(L / (FINE_THREADS * FINE_U)): passes of a workgroup over its frame
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // ceil(L / STUDY_ACC_COLS) + 1
  size_t acc_lds;            // static LDS of the accumulating kernel
};

inline FinePass fine_pass(const TxfShape& s, int variant, int64_t frames) {
  const int64_t L = fine_len(s.np, s.n_symb, variant);
  FinePass p{};
  p.threads = FINE_THREADS;
  p.grid = (unsigned)frames;
  p.lds = FINE_SCRATCH_BYTES;
  p.trips = (int)((L + FINE_THREADS * FINE_U - 1) / (FINE_THREADS * FINE_U));
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(L, 1);
  p.acc_lds = STUDY_ACC_LDS;
  return p;
}

}  // namespace ofdm
