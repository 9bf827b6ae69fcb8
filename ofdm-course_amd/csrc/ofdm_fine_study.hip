// The fine-sync capture: `taus`, the per-pilot-pair residual-delay estimate of fine_sync (T4/fine_sync.m:10-30, T5/fine_sync.m:8-16;
// figures 18a / 18b of the Task-4 report plot it over the carrier number) with the mask of T4 :33 / T5 :18, the two estimates
// (:35 / :20, :52 / :37) and their denominators for every frame, and the tau(SNR) study of T4/Main_model_Task_4.m:137-203.
//
//   fine_capture_kernel<T>    one workgroup of FS_THREADS per frame runs fine_tau_body and fine_phase_body (sync_core.hpp) with
//                             their capture on: the arithmetic -- tau_of, angle0_t, fine_rot, the rank rule, the order of the two
//                             reductions -- is the receiver's and ofdm_fine_sync's, so tau and phase are theirs bit for bit; each
//                             thread's FS_U consecutive `taus` values and keep flags go to the frame's rows in the trip that forms
//                             them.  Thread 0 ends with the frame's scalars and, in the study, the frame's timing error
//                             (fine_tau_err) and the increments of the point's integer tables (atomics on integers).
//   fine_accumulate_kernel    one thread per entry adds: sums[i] = (..(sums[i] + t_0[i]) + t_1[i]) + .. over the chunk's rows in
//                             frame order (the rows staged through LDS by the whole workgroup), a value that is not finite counted
//                             in dropped[i] instead, and counts the frames whose entry passed the mask.  Its last workgroup adds
//                             the chunk's timing errors and common phases in frame order to {sum |e|, sum e^2}, {sum ph, sum ph^2}.
//                             The chunks of a point run in stream order on accumulators the call zeroed, so every double is
//                             ((0 + v_0) + v_1) + .. whatever the chunking.
// ofdm_fine_study generates each chunk with the fused generator (txf_sweep_points, the RX frames in the plan-owned workspace), runs the
// front end of the Task-4 receiver on it (task4_front_end, ofdm_chain_t4.hip: the stages task4_run itself runs in front of
// fine_sync, on the route of t4_route.hpp) and then the two kernels on the pilot rows the demodulator left; no equaliser, no
// demapper.  Host side: the checks, the chunk and the launch shape are fine_plan.hpp's, plain C++ tested without a GPU.
#include <algorithm>
#include <cmath>

#include "fine_plan.hpp"
#include "study_accumulate.hpp"
#include "sync_core.hpp"
#include "txf_study.hpp"

namespace ofdm {

static_assert(FINE_THREADS == FS_THREADS && FINE_U == FS_U && FINE_SCRATCH_BYTES == sizeof(FsScratch), "fine_plan.hpp restates sync_core.hpp");

// what a frame's workgroup leaves behind; taus / keep may be null, and the study's block is used where tau_hist is given
struct FineOut {
  double* taus;              // [frames][L]
  uint8_t* keep;             // [frames][L]
  double *tau, *phase;       // [frames]
  int32_t *n_used, *n_phase; // [frames]
  // the study: the front end's TgPosition, the frame's Time_Delay draw (null: 0), the point's tables, the chunk's errors
  const int64_t *tg, *sto;
  unsigned long long *tau_hist, *tau_below, *tau_above, *tau_nan, *phase_nan, *used_sum, *tg_hist;
  double* err;
  int bins_n;
  double bins_lo, bins_hi;
  int nfft, stride;
};

template <typename T>
__global__ __launch_bounds__(FS_THREADS) void fine_capture_kernel(PilotView<T> pv, double deltak, int variant, int time_desync, int64_t L,
                                                                  FineOut o) {
  __shared__ FsScratch sc;
  const int64_t f = blockIdx.x;
  pv.rx += f * pv.rx_fstride;
  const FsCapture cap{o.taus ? o.taus + f * L : nullptr, o.keep ? o.keep + f * L : nullptr, o.n_used + f, o.n_phase + f};
  const double tau = fine_tau_body<T, FsCapture>(pv, deltak, variant, sc, cap);
  const double ph = fine_phase_body<T, FsCapture>(pv, time_desync, tau, sc, nullptr, cap);
  if (threadIdx.x != 0) return;
  o.tau[f] = tau;
  o.phase[f] = ph;
  if (!o.tau_hist) return;
  const int64_t tg = o.tg[f], sto = o.sto ? o.sto[f] : 0;
  const double e = fine_tau_err(tau, tg, sto, o.nfft, o.stride);
  o.err[f] = e;
  const int b = fine_bin(e, o.bins_n, o.bins_lo, o.bins_hi);
  atomicAdd(b >= 0 ? o.tau_hist + b : b == FINE_BIN_BELOW ? o.tau_below : b == FINE_BIN_ABOVE ? o.tau_above : o.tau_nan, 1ull);
  if (!(ph - ph == 0.0)) atomicAdd(o.phase_nan, 1ull);
  atomicAdd(o.used_sum, (unsigned long long)o.n_used[f]);       // thread 0 wrote it
  atomicAdd(o.tg_hist + sync_phase_bin(tg, sto, o.stride), 1ull);
}

// rows / keep [nf][L] of a chunk into the point's sums / dropped / keep_counts [L]; err / phase [nf] into tau_err / phase_sums [2]:
// the column workgroups of study_accumulate.hpp, a value that is not finite dropped, the keep bytes counted; the tail workgroup
// takes the two columns of per-frame scalars, the values that are not finite left out.
__global__ __launch_bounds__(STUDY_ACC_THREADS) void fine_accumulate_kernel(const double* __restrict__ rows, const uint8_t* __restrict__ keep,
                                                                            const double* __restrict__ err, const double* __restrict__ phase,
                                                                            int64_t nf, int64_t L, double* __restrict__ sums,
                                                                            unsigned long long* __restrict__ dropped,
                                                                            unsigned long long* __restrict__ keep_counts,
                                                                            double* __restrict__ tau_err, double* __restrict__ phase_sums) {
  __shared__ StudyAccTile tile;
  if (blockIdx.x == gridDim.x - 1) return study_accumulate_scalars<true, true>(tile, err, phase, nf, tau_err, phase_sums);
  study_accumulate_columns<true, ACC_PEAK_OFF, true>(tile, rows, nullptr, keep, nf, L, sums, dropped, nullptr, keep_counts);
}

// the capture over nf frames whose pilot rows are `rows` (device memory, the plan's precision)
template <typename T>
static int fine_capture_frames(const ofdm_rx_plan* pl, const TxfShape& s, const T4PilotRows& v, int64_t nf, int variant, int time_desync,
                               const FineOut& o) {
  const FinePass p = fine_pass(s, variant, nf);
  const int64_t L = fine_len(s.np, s.n_symb, variant);
  const double deltak = (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0];                 // fine_sync.m:6
  PilotView<T> pv{(const cx<T>*)v.rows, (const cx<T>*)v.tx, (const int32_t*)pl->d_pc0, s.nfft, s.np, (int64_t)s.np * s.n_symb, v.fstride,
                  v.compact};
  hipLaunchKernelGGL(fine_capture_kernel<T>, dim3(p.grid), dim3(p.threads), 0, ctx().stream, pv, deltak, variant, time_desync, L, o);
  return check_launch("fine_capture_kernel");
}

static int fine_capture_any(const ofdm_rx_plan* pl, const TxfShape& s, const T4PilotRows& v, int64_t nf, int variant, int time_desync,
                            const FineOut& o) {
  return pl->f64 ? fine_capture_frames<double>(pl, s, v, nf, variant, time_desync, o)
                 : fine_capture_frames<float>(pl, s, v, nf, variant, time_desync, o);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_fine(ofdm_rx_plan* pl, const void* x, int64_t n_frames, int variant, int time_desync, double* taus_out,
                            uint8_t* keep_out, double* tau_out, double* phase_out, int32_t* n_used_out, int32_t* n_phase_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  FineCapture cap;
  cap.variant = variant;
  cap.out = taus_out || keep_out || tau_out || phase_out || n_used_out || n_phase_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(fine_rx_prelude(pl ? &s : nullptr, x != nullptr, is_f64(flags), n_frames, cap, why), why));
  if (n_frames == 0) return OFDM_OK;
  const size_t nf = (size_t)n_frames, grid = (size_t)pl->nfft * pl->n_symb, L = (size_t)fine_len(s.np, s.n_symb, variant);
  Stage st(flags);
  const void* dx;
  void *dtaus, *dkeep, *dtau, *dph, *dnu, *dnp;
  OFDM_TRY(st.in(x, csize(flags) * grid * nf, &dx));
  OFDM_TRY(st.out(taus_out, sizeof(double) * L * nf, &dtaus));
  OFDM_TRY(st.out(keep_out, L * nf, &dkeep));
  // the scalars are always produced (scratch when the caller does not want them)
  auto scalar = [&st](void* user, size_t bytes, void** d) { return user ? st.out(user, bytes, d) : st.scratch(bytes, d); };
  OFDM_TRY(scalar(tau_out, sizeof(double) * nf, &dtau));
  OFDM_TRY(scalar(phase_out, sizeof(double) * nf, &dph));
  OFDM_TRY(scalar(n_used_out, sizeof(int32_t) * nf, &dnu));
  OFDM_TRY(scalar(n_phase_out, sizeof(int32_t) * nf, &dnp));
  T4PilotRows v{dx, nullptr, (int64_t)grid, 0};
  OFDM_TRY(task4_pilot_matrix(pl, &v.tx));
  FineOut o{};
  o.taus = (double*)dtaus; o.keep = (uint8_t*)dkeep; o.tau = (double*)dtau; o.phase = (double*)dph;
  o.n_used = (int32_t*)dnu; o.n_phase = (int32_t*)dnp;
  OFDM_TRY(fine_capture_any(pl, s, v, n_frames, variant, time_desync ? 1 : 0, o));
  return st.finish();
}

extern "C" int ofdm_fine_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                               int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                               int freq_desync, int variant, const uint8_t* scr_reg15, const double* snr_db, const uint64_t* seeds,
                               int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk, int bins_n,
                               double bins_lo, double bins_hi, double* tau_curve_sums_out, uint64_t* curve_dropped_out,
                               uint64_t* keep_counts_out, uint64_t* tau_hist_out, uint64_t* tau_below_out, uint64_t* tau_above_out,
                               uint64_t* tau_nan_out, double* tau_err_out, double* phase_sums_out, uint64_t* phase_nan_out,
                               uint64_t* used_sums_out, uint64_t* tg_hist_out, double* frame_tau_out, double* frame_phase_out,
                               int32_t* frame_n_used_out, int64_t* frame_tg_out, int32_t* frame_status_out,
                               int64_t* frame_time_delay_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs a{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  FineCapture cap;
  cap.variant = variant;
  cap.out = tau_curve_sums_out || curve_dropped_out || keep_counts_out || tau_hist_out || tau_below_out || tau_above_out || tau_nan_out ||
            tau_err_out || phase_sums_out || phase_nan_out || used_sums_out || tg_hist_out || frame_tau_out || frame_phase_out ||
            frame_n_used_out || frame_tg_out || frame_status_out || frame_time_delay_out;
  FineBins bins;
  bins.n = bins_n; bins.lo = bins_lo; bins.hi = bins_hi;
  const int td = time_desync ? 1 : 0, fd = freq_desync ? 1 : 0;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(fine_study_prelude(a.call("fine_study", pl ? &s : nullptr), a.both_channels(), td, fd, cap, bins, ch, fade.gains,
                                          why), why));
  const int stride = pl->nfft + pl->t_guard;
  const int64_t L = fine_len(s.np, s.n_symb, variant);
  const size_t np = (size_t)n_points, fpp = (size_t)frames_per_point, Ls = (size_t)L;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  TxfFrameOut<double> ftau, fph;
  TxfFrameOut<int32_t> fnu, fst;
  TxfFrameOut<int64_t> ftg, ftd;
  OFDM_TRY(ftau.out(st, frame_tau_out, np * fpp));
  OFDM_TRY(fph.out(st, frame_phase_out, np * fpp));
  OFDM_TRY(fnu.out(st, frame_n_used_out, np * fpp));
  OFDM_TRY(ftg.out(st, frame_tg_out, np * fpp));
  OFDM_TRY(fst.out(st, frame_status_out, np * fpp));
  OFDM_TRY(ftd.out(st, frame_time_delay_out, np * fpp));
  if (n_points == 0) return st.finish();
  double *dsums, *dterr, *dpsum;
  unsigned long long *ddrop, *dkeepc, *dhist, *dbelow, *dabove, *dnan, *dpnan, *dused, *dtgh;
  OFDM_TRY(txf_table(st, tau_curve_sums_out, Ls * np, dsums));
  OFDM_TRY(txf_table(st, curve_dropped_out, Ls * np, ddrop));
  OFDM_TRY(txf_table(st, keep_counts_out, Ls * np, dkeepc));
  OFDM_TRY(txf_table(st, tau_hist_out, (size_t)bins_n * np, dhist));
  OFDM_TRY(txf_table(st, tau_below_out, np, dbelow));
  OFDM_TRY(txf_table(st, tau_above_out, np, dabove));
  OFDM_TRY(txf_table(st, tau_nan_out, np, dnan));
  OFDM_TRY(txf_table(st, tau_err_out, 2 * np, dterr));
  OFDM_TRY(txf_table(st, phase_sums_out, 2 * np, dpsum));
  OFDM_TRY(txf_table(st, phase_nan_out, np, dpnan));
  OFDM_TRY(txf_table(st, used_sums_out, np, dused));
  OFDM_TRY(txf_table(st, tg_hist_out, (size_t)stride * np, dtgh));
  if (frames_per_point == 0) return st.finish();
  const bool imp_on = a.imp_on();
  const TxfUse u = a.use(ch);
  const int64_t CH = fine_chunk(s, u, frames_per_point, max_frames_per_chunk, variant);
  const size_t chn = (size_t)CH;
  void *rows, *keepm, *err, *cnp, *cfo, *cifo;
  OFDM_TRY(st.scratch(sizeof(double) * Ls * chn, &rows));
  OFDM_TRY(st.scratch(Ls * chn, &keepm));
  OFDM_TRY(st.scratch(sizeof(double) * chn, &err));
  OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &cnp));
  OFDM_TRY(st.scratch(sizeof(double) * chn, &cfo));
  OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &cifo));
  OFDM_TRY(ftau.scratch(st, chn));
  OFDM_TRY(fph.scratch(st, chn));
  OFDM_TRY(fnu.scratch(st, chn));
  OFDM_TRY(ftg.scratch(st, chn));
  OFDM_TRY(fst.scratch(st, chn));
  const TxfImp imp = a.imp();
  OFDM_TRY(txf_sweep_points(pl, ch, a.points(), scr_reg15, CH, imp_on ? &imp : nullptr, a.fading() ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    T4PilotRows v{};
    OFDM_TRY(task4_front_end(pl, b.rx, nf, td, fd, ftg.at(at), (double*)cfo, (int32_t*)cifo, fst.at(at), &v));
    if (ftd.sweep) {                                                      // (no scratch: written only where the caller wants it)
      if (imp_on) OFDM_HIP(hipMemcpyAsync(ftd.at(at), b.sto, sizeof(int64_t) * (size_t)nf, hipMemcpyDeviceToDevice, stream));
      else OFDM_HIP(hipMemsetAsync(ftd.at(at), 0, sizeof(int64_t) * (size_t)nf, stream));
    }
    FineOut o{};
    o.taus = (double*)rows; o.keep = (uint8_t*)keepm;
    o.tau = ftau.at(at); o.phase = fph.at(at); o.n_used = fnu.at(at);
    o.n_phase = (int32_t*)cnp;
    o.tg = ftg.at(at); o.sto = imp_on ? b.sto : nullptr;
    o.tau_hist = dhist + (size_t)bins_n * p; o.tau_below = dbelow + p; o.tau_above = dabove + p; o.tau_nan = dnan + p;
    o.phase_nan = dpnan + p; o.used_sum = dused + p; o.tg_hist = dtgh + (size_t)stride * p;
    o.err = (double*)err;
    o.bins_n = bins_n; o.bins_lo = bins_lo; o.bins_hi = bins_hi;
    o.nfft = pl->nfft; o.stride = stride;
    OFDM_TRY(fine_capture_any(pl, s, v, nf, variant, td, o));
    const FinePass fp = fine_pass(s, variant, nf);
    hipLaunchKernelGGL(fine_accumulate_kernel, dim3(fp.acc_grid), dim3(fp.acc_threads), 0, stream, (const double*)rows,
                       (const uint8_t*)keepm, (const double*)err, (const double*)o.phase, nf, L, dsums + Ls * p, ddrop + Ls * p,
                       dkeepc + Ls * p, dterr + 2 * p, dpsum + 2 * p);
    return check_launch("fine_accumulate_kernel");
  }));
  return st.finish();
}
