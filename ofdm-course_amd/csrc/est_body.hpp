// The four estimators of Task 5 on a batch of received frames (ofdm_part2.hip): from "received frames drx[F]" to "four H buffers
// and four error rows".  One body for its users: ofdm_task5_part2_tile, ofdm_task5_mse_tile and, through est_study_run
// (ofdm_est_study.hip), ofdm_estimator_study and ofdm_estimator_profile.  What differs between them is in front of it (how the frames were made) and in EstBodyArgs.
#pragma once

#include "rx_plan.hpp"

namespace ofdm {

struct EstBodyArgs {
  const char* what;              // the entry as its refusals name it
  int mmse_max_np;               // the pilots the entry's MMSE stage takes (585: four wavefronts per workgroup; 2400: what one holds in LDS)
  int mmse_named_np;             // the count the entry's refusal has always named (the MSE tile says 2343 for its bound of 2400)
  const void* ref;               // packed reference bits of every frame [F][frame_words]; null: no equaliser runs, H of MP / OMP
                                 // is the transform of their taps (mse_taps_to_h_kernel) and errs is not written
  uint32_t* errs;                // [4][F] bit errors, rows LS, MMSE, MP, OMP
  const double* cvals;           // [F] c = 2 pi tau_rms df Nps of MMSE_CE.m:19-26; null: from h = ifft(H_LS) of the frame
                                 // (Main_model_Task_5.m:314-315, mse_tau_kernel)
  double inv_snr;                // 1 / snr of every frame (MMSE_CE.m:13), or
  const double* inv_snr_v;       // [F], each frame at its own
};

// the body's share of the plan's arena (ws_t4) behind `front` bytes of the caller's; est_plan.hpp budgets est_body_frame_bytes
size_t est_body_bytes(const ofdm_rx_plan* pl, int64_t F);
int est_arena(ofdm_rx_plan* pl, size_t front, int64_t F, unsigned char** front_out, unsigned char** body_out);

// what the body refuses, before anything is launched: N_carrier of mse_tau_kernel (ls_tau: c is not given), np <= mmse_max_np,
// k_atoms >= np for MP, the MP stage's LDS
int est_body_check(const ofdm_rx_plan* pl, const char* what, int mmse_max_np, int mmse_named_np, bool ls_tau);

template <typename T>
struct EstBodyOut {
  cx<T>* h[4];                   // [F][N_carrier] each: LS, MMSE, MP, OMP
  const int32_t* tap_idx;        // [F][taps] the plan's tap workspace as the body leaves it: OMP's picks, 0-based, -1 = not made
  const c64* tap_x;              // [F][taps] their coefficients (a pick repeated later holds 0 in its earlier slot)
};

// drx: [F][(Nfft + T_guard) N_symb] received frames in the plan's precision; body: est_arena's body_out
template <typename T>
int est_body_run(ofdm_rx_plan* pl, const EstBodyArgs& a, const void* drx, int64_t F, unsigned char* body, EstBodyOut<T>& out);

}  // namespace ofdm
