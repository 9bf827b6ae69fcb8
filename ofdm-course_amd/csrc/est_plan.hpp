// The plan of one call of the estimator study (ofdm_est_study.hip): ofdm_estimator_study, the comparison of Task 5 -- LS_CE,
// MMSE_CE, MP_estimate and OMP_estimate on the same received frame of every channel realisation (T5/Task5_part2.m:148-205,
// :269-304; over SNR T5/Main_model_Task_5.m:303-346) -- per point of a sweep of the fused generator: four bit-error counts and
// four channel-estimate error sums.  The argument checks in the order they are made, the chunk the generator's workspace and the
// estimator body's arena (est_body.hpp) allow, and the launch shape of the study's own kernels.  Plain C++ with no device or
// runtime dependency: tests/host/est_plan_main.cpp runs it under the host sanitizers.  The .hip side turns a refusal into
// OFDM_ERR_ARG (TXF_REFUSE_DEVICE: OFDM_ERR_STATE) with TxfWhy::text as the last-error string.
#pragma once

#include <cstddef>
#include <cstdint>

#include "txf_plan.hpp"

namespace ofdm {

constexpr int EST_ROWS = 4;                           // LS, MMSE, MP, OMP: the order of every [4] of the study
enum { EST_ROW_LS, EST_ROW_MMSE, EST_ROW_MP, EST_ROW_OMP };
enum { EST_TAU_LS = 0, EST_TAU_GENIE = 1 };           // mmse_mode: h = ifft(H_LS) per frame / the frame's true taps

// the refusals of the entry: a TXF_REFUSE_* of txf_plan.hpp, or one of its own
enum { EST_REFUSE_BOTH = TXF_REFUSALS, EST_REFUSE_DESCR, EST_REFUSE_MMSE_MODE, EST_REFUSE_OUTPUT, EST_REFUSALS };

struct EstWanted {
  int mmse_mode = EST_TAU_LS;
  bool out = false;          // an output is given
};

// The order of the checks; the first that fails is the refusal a caller sees.
//   the front every study shares (txf_study_prelude: bad arguments, max_frames_per_chunk 0 .. 65535 -- the equalise stage's limit
//   --, snr_db / seeds, too many points, the plan -- device, precision, data carriers, pilots in band, Nfft / T_guard, the streams
//   of one point --, h and taps together, the channel) -> a plan with a DeScrambler (the study runs unscrambled, as
//   Task5_part2.m:104-114 does; the entry takes no Register) -> mmse_mode 0 / 1 -> an output is given.
// The generator needs data carriers, so a plan without them (comb 1) is the front's refusal whatever the outputs.
// WHAT: the entry as its refusals name it (ofdm_estimator_profile, est_profile_plan.hpp, makes the same checks under its own name).
inline int est_study_prelude(const TxfCall& c, bool both_channels, const EstWanted& e, TxfChannel& ch, TxfGains& g, TxfWhy& w,
                             const char* WHAT = "estimator_study") {
  if (const int id = txf_study_prelude(c, both_channels, EST_REFUSE_BOTH, WHAT, ch, g, w, 65535)) return id;
  if (c.plan->descr & TXF_DESCR_ON)
    return txf_refuse(w, EST_REFUSE_DESCR,
                      "%s: the study runs unscrambled (Task5_part2.m:104-114,:285-299 are commented out); clear the plan's DeScrambler", WHAT);
  if (!(e.mmse_mode == EST_TAU_LS || e.mmse_mode == EST_TAU_GENIE))
    return txf_refuse(w, EST_REFUSE_MMSE_MODE, "%s: mmse_mode must be 0 (h = ifft(H_LS)) or 1 (the frame's true taps) (%d)", WHAT, e.mmse_mode);
  if (!e.out) return txf_refuse(w, EST_REFUSE_OUTPUT, "%s: no output is given", WHAT);
  return TXF_OK;
}

// ---- the chunk: frames of one point.  Beside the generator's regions, per frame
//   the estimator body's arena (est_body.hpp)   X(1..N_carrier, :) of every symbol, v [Np], c, four H [N_carrier]
//   the plan's pilot workspace                   X(1..N_carrier, 1), Y [Np], the picks and coefficients of `taps` paths
//   the study's rows                             the true H [N_carrier] in double, the body's four error rows, four error sums
// on twice the workspace budget, as the studies behind the Task-4 receiver (which shares the arena) budget theirs.
inline size_t est_body_frame_bytes(const TxfShape& s) {
  const size_t cs = s.f64 ? 16 : 8;
  return cs * ((size_t)s.n_carrier * s.n_symb + (size_t)s.np + EST_ROWS * (size_t)s.n_carrier) + sizeof(double);
}

inline size_t est_row_bytes(const TxfShape& s, int taps) {
  const size_t cs = s.f64 ? 16 : 8;
  return cs * ((size_t)s.n_carrier + (size_t)s.np) + (sizeof(int32_t) + 16) * (size_t)taps + 16 * (size_t)s.n_carrier +
         EST_ROWS * (sizeof(uint32_t) + sizeof(double));
}

inline int64_t est_chunk(const TxfShape& s, const TxfUse& u, int taps, int64_t frames_per_point, int64_t user_cap,
                         size_t budget = 2 * TXF_WS_BUDGET) {
  return txf_chunk(s, u, frames_per_point, user_cap, budget, est_body_frame_bytes(s) + est_row_bytes(s, taps));
}

// ---- the launch shape.  est_truth_kernel and est_reduce_kernel: one workgroup of EST_THREADS threads per frame of the chunk, the
// carriers across the threads with a stride of EST_THREADS.  The truth kernel stages the frame's taps (16 TXF_MAX_TAPS bytes; one
// thread forms the three moments of c serially); the reduce kernel keeps the four partials of each wavefront and nothing else.  The in-order sums
// are the studies' accumulate shape over EST_ROWS columns: one workgroup.
constexpr int EST_THREADS = 256;
constexpr int EST_WAVES = EST_THREADS / 64;
constexpr size_t EST_TRUTH_LDS = 16 * (size_t)TXF_MAX_TAPS;
constexpr size_t EST_REDUCE_LDS = sizeof(double) * EST_ROWS * EST_WAVES;

static_assert(EST_TRUTH_LDS == 1024 && EST_REDUCE_LDS == 128, "the study kernels' LDS");

struct EstPass {
  int threads;               // EST_THREADS
  unsigned grid;             // frames of the chunk
  size_t truth_lds, reduce_lds;
  int acc_threads;           // STUDY_ACC_THREADS
  unsigned acc_grid;         // study_acc_grid(EST_ROWS, 0) = 1
};

inline EstPass est_pass(int64_t frames) {
  EstPass p{};
  p.threads = EST_THREADS;
  p.grid = (unsigned)frames;
  p.truth_lds = EST_TRUTH_LDS;
  p.reduce_lds = EST_REDUCE_LDS;
  p.acc_threads = STUDY_ACC_THREADS;
  p.acc_grid = study_acc_grid(EST_ROWS, 0);
  return p;
}

}  // namespace ofdm
