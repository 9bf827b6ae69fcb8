// The estimator study: LS_CE, MMSE_CE, MP_estimate and OMP_estimate on the same received frame of every channel realisation
// (T5/Task5_part2.m:148-205, :269-304; over SNR T5/Main_model_Task_5.m:303-346), per point of a sweep of the fused generator: four
// bit-error counts and four channel-estimate error sums, every estimator behind the same noise and the same channel.
//
//   est_truth_kernel       one workgroup per frame of the chunk: the true H_f(k) = fft(h_f)(k) on carriers 1..N_carrier in double
//                          (channel_resp, the H the sweeps' error sum sees), from the frame's own tap amplitudes (a channel per frame)
//                          or, once per call, from the static channel's.  mmse = genie: also c_f = 2 pi tau_rms df Nps of the frame's
//                          taps by the rule ofdm_task5_part2_tile applies on the host (MMSE_CE.m:19-24 on h(1:N_carrier): taps with a
//                          delay below N_carrier, in tap order, r2 - r^2 clamped by mmse_tau.hpp); a frame with no such tap gets NaN,
//                          which carries through its MMSE row into nmse_dropped.  The truth is double whatever the plan's precision,
//                          so the kernel has no precision parameter.
//   est_reduce_kernel<T>   one workgroup per frame: sum_k |H_f(k) - H_e,f(k)|^2 of the four estimates in double, in the order of
//                          t5_frame_nmse_kernel (a stride of 256 per thread, the butterfly of a wavefront, the four wave partials
//                          paired) -> frame_nmse[f][4]; the body's four error rows -> errors[p][4] (integer atomics) and
//                          frame_errors[f][4].  LDS: the four partials of each wavefront.
//   est_accumulate_kernel  the workgroups of one launch have no order, so the in-order sum is a launch of its own: the studies'
//                          column body (study_accumulate.hpp) over the chunk's rows frame_nmse[nf][4] into nmse_sums[p][4], a
//                          value that is not finite left out and counted in nmse_dropped[p][4].  The chunks of a point run in
//                          stream order on accumulators the call zeroed: ((0 + v_0) + v_1) + .. whatever the chunking.
// ofdm_estimator_study generates each chunk with the fused generator (txf_sweep_points) and runs the estimator body of the two
// Task-5 tiles on it (est_body_run, ofdm_part2.hip) with the generator's per-frame reference bits.  mmse = ls: the body's own
// h = ifft(H_LS) stage (mse_tau_kernel) at the point's SNR (Main_model_Task_5.m:314-315).  The receiver and its route are not
// involved.  Host side: the checks, the chunk and the launch shapes are est_plan.hpp's; the body's refusals come in the part-2
// tile's words.  The call itself is est_study_run (est_study.hpp), which ofdm_estimator_profile (ofdm_est_profile.hip) shares: the
// same frames, the same launches in the same order, and its own kernels behind each chunk.
#include <algorithm>
#include <cmath>

#include "est_body.hpp"
#include "est_plan.hpp"
#include "est_study.hpp"
#include "mmse_tau.hpp"
#include "study_accumulate.hpp"
#include "txf_study.hpp"

namespace ofdm {

__global__ __launch_bounds__(EST_THREADS) void est_truth_kernel(const c64* __restrict__ amp, int64_t amp_stride, TxfDelays dl, int nfft,
                                                                int n_carrier, c64* __restrict__ htrue, double nps,
                                                                double* __restrict__ cvals) {
  __shared__ c64 a[TXF_MAX_TAPS];
  const int64_t f = blockIdx.x;
  if ((int)threadIdx.x < dl.n) a[threadIdx.x] = amp[f * amp_stride + threadIdx.x];
  __syncthreads();
  if (amp_stride != 0 || f == 0) {                    // a static channel: one row, written by the first workgroup
    const double inv = 2.0 / (double)nfft;
    c64* const row = htrue + (amp_stride != 0 ? f * n_carrier : 0);
    for (int k = threadIdx.x; k < n_carrier; k += EST_THREADS) {
      double hr, hi;
      channel_resp(a, dl, k, nfft, inv, hr, hi);
      row[k] = mk<double>(hr, hi);
    }
  }
  if (cvals && threadIdx.x == 0) {
    // the rule of ofdm_task5_part2_tile's host loop, the taps in their order; the device may contract where the host does not,
    // so c agrees with the tile's to rounding, not bit for bit
    double hh = 0, s1 = 0, s2 = 0;
    for (int t = 0; t < dl.n; ++t) {
      const int d = dl.d[t];
      if (d >= n_carrier) continue;                   // h(1:N_carrier)
      const double p = a[t].x * a[t].x + a[t].y * a[t].y;
      hh += p; s1 += p * d; s2 += p * (double)d * d;
    }
    cvals[f] = hh > 0 ? mmse_tau_c(hh, s1, s2, 1.0 / (double)n_carrier, nps) : NAN;
  }
}

template <typename T>
struct EstRows {
  const cx<T>* h[EST_ROWS];
};

template <typename T>
__global__ __launch_bounds__(EST_THREADS) void est_reduce_kernel(const c64* __restrict__ htrue, int64_t h_stride, EstRows<T> est,
                                                                 int n_carrier, const uint32_t* __restrict__ errs, int64_t nf,
                                                                 double* __restrict__ frame_nmse,
                                                                 unsigned long long* __restrict__ errors,
                                                                 uint32_t* __restrict__ frame_errors) {
  __shared__ double part[EST_ROWS][EST_WAVES];
  const int64_t f = blockIdx.x;
  double acc[EST_ROWS] = {0, 0, 0, 0};
  for (int k = threadIdx.x; k < n_carrier; k += EST_THREADS) {
    const c64 t = htrue[f * h_stride + k];
#pragma unroll
    for (int e = 0; e < EST_ROWS; ++e) {
      const cx<T> he = est.h[e][f * n_carrier + k];
      const double dr = t.x - (double)he.x, di = t.y - (double)he.y;
      acc[e] += dr * dr + di * di;
    }
  }
#pragma unroll
  for (int e = 0; e < EST_ROWS; ++e) {
    double v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) part[e][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < EST_ROWS) {
    const int e = threadIdx.x;
    frame_nmse[f * EST_ROWS + e] = (part[e][0] + part[e][1]) + (part[e][2] + part[e][3]);
    if (errs) {
      const uint32_t n = errs[e * nf + f];
      if (frame_errors) frame_errors[f * EST_ROWS + e] = n;
      if (n) atomicAdd(errors + e, (unsigned long long)n);
    }
  }
}

__global__ __launch_bounds__(STUDY_ACC_THREADS) void est_accumulate_kernel(const double* __restrict__ rows, int64_t nf,
                                                                          double* __restrict__ sums,
                                                                          unsigned long long* __restrict__ dropped) {
  __shared__ StudyAccTile tile;
  study_accumulate_columns<true, ACC_PEAK_OFF, false>(tile, rows, nullptr, nullptr, nf, EST_ROWS, sums, dropped, nullptr, nullptr);
}

// the true channel of nf frames (amp_stride 0: of the static channel, one row) and, with cvals, their c
static int est_truth(const ofdm_rx_plan* pl, const c64* amp, int64_t amp_stride, const TxfDelays& dl, int64_t nf, c64* htrue,
                     double* cvals) {
  const EstPass p = est_pass(nf);
  const double nps = (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0];       // MMSE_CE.m:15
  hipLaunchKernelGGL(est_truth_kernel, dim3(p.grid), dim3(p.threads), 0, ctx().stream, amp, amp_stride, dl, pl->nfft, pl->n_carrier, htrue,
                     nps, cvals);
  return check_launch("est_truth_kernel");
}

template <typename T>
static int est_chunk_run(ofdm_rx_plan* pl, const EstBodyArgs& a, const void* drx, int64_t nf, unsigned char* body, const c64* htrue,
                         int64_t h_stride, double* frame_nmse, unsigned long long* errors, uint32_t* frame_errors, double* sums,
                         unsigned long long* dropped, EstChunkDone& done) {
  EstBodyOut<T> o;
  OFDM_TRY(est_body_run<T>(pl, a, drx, nf, body, o));
  const EstPass p = est_pass(nf);
  const EstRows<T> rows{{o.h[0], o.h[1], o.h[2], o.h[3]}};
  hipLaunchKernelGGL(est_reduce_kernel<T>, dim3(p.grid), dim3(p.threads), 0, ctx().stream, htrue, h_stride, rows, pl->n_carrier,
                     a.ref ? (const uint32_t*)a.errs : nullptr, nf, frame_nmse, errors, frame_errors);
  OFDM_TRY(check_launch("est_reduce_kernel"));
  hipLaunchKernelGGL(est_accumulate_kernel, dim3(p.acc_grid), dim3(p.acc_threads), 0, ctx().stream, (const double*)frame_nmse, nf, sums,
                     dropped);
  for (int e = 0; e < EST_ROWS; ++e) done.h[e] = o.h[e];
  done.tap_idx = o.tap_idx;
  done.tap_x = o.tap_x;
  return check_launch("est_accumulate_kernel");
}

int est_study_run(const EstStudyCall& call, EstStudyHook* hook) {
  ofdm_rx_plan* const pl = call.pl;
  const TxfStudyArgs& g = call.g;
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const bool fading = g.fading();
  EstWanted want;
  want.mmse_mode = call.mmse_mode;
  want.out = call.errors_out || call.nmse_sums_out || call.nmse_dropped_out || call.frame_errors_out || call.frame_nmse_out ||
             (hook && hook->out());
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  const TxfCall front = g.call(hook ? hook->what() : "estimator_study", pl ? &s : nullptr);
  OFDM_TRY(txf_refused(hook ? hook->prelude(front, g.both_channels(), want, ch, fade.gains, why)
                            : est_study_prelude(front, g.both_channels(), want, ch, fade.gains, why), why));
  // what the part-2 tile refuses of a plan, in its words, before anything is written
  const bool want_err = call.errors_out || call.frame_errors_out;
  const bool genie = call.mmse_mode == EST_TAU_GENIE;
  EstBodyArgs ba{"task5_part2_tile", 585, 585, nullptr, nullptr, nullptr, 0.0, nullptr};
  OFDM_ARG(pl->np >= 2, "task5_part2_tile: needs at least two pilots, all inside 1..N_carrier");
  OFDM_ARG(!want_err || chain_split_fits(pl->taps, pl->bps, pl->n_carrier, (int64_t)pl->nd * pl->n_symb, pl->f64 != 0),
           "task5_part2_tile: the frame's decisions do not fit the equalise stage's LDS");
  OFDM_TRY(est_body_check(pl, ba.what, ba.mmse_max_np, ba.mmse_named_np, !genie));
  if (g.n_points == 0) return OFDM_OK;
  const size_t np = (size_t)g.n_points, fpp = (size_t)g.frames_per_point, nc = (size_t)pl->n_carrier;
  Stage st(g.flags);
  unsigned long long *derr, *ddrop;
  double* dsum;
  TxfFrameOut<uint32_t> fe;
  TxfFrameOut<double> fn;
  OFDM_TRY(txf_table(st, call.errors_out, EST_ROWS * np, derr));
  OFDM_TRY(txf_table(st, call.nmse_sums_out, EST_ROWS * np, dsum));
  OFDM_TRY(txf_table(st, call.nmse_dropped_out, EST_ROWS * np, ddrop));
  OFDM_TRY(fe.out(st, call.frame_errors_out, EST_ROWS * np * fpp));
  OFDM_TRY(fn.out(st, call.frame_nmse_out, EST_ROWS * np * fpp));
  if (hook) OFDM_TRY(hook->tables(st, np, fpp));
  if (g.frames_per_point == 0) return st.finish();
  const int taps = (int)ch.delay.size();
  const TxfUse u = g.use(ch);
  const int64_t CH = hook ? hook->chunk(s, u, pl->taps, g.frames_per_point, g.max_frames_per_chunk)
                          : est_chunk(s, u, pl->taps, g.frames_per_point, g.max_frames_per_chunk);
  const size_t chn = (size_t)CH;
  OFDM_TRY(fn.scratch(st, EST_ROWS * chn));
  void *dtrue, *dcv = nullptr, *drows = nullptr, *dstatic = nullptr;
  OFDM_TRY(st.scratch(sizeof(c64) * nc * (fading ? chn : 1), &dtrue));
  if (genie) OFDM_TRY(st.scratch(sizeof(double) * chn, &dcv));
  if (want_err) OFDM_TRY(st.scratch(sizeof(uint32_t) * EST_ROWS * chn, &drows));
  unsigned char *front_bytes, *body;
  OFDM_TRY(est_arena(pl, 0, CH, &front_bytes, &body));
  const TxfDelays dl = txf_delays(ch);
  if (hook) OFDM_TRY(hook->begin(st, dl, CH));
  if (!fading) {                                                  // a static channel: its taps, its H(k) and its c, once
    OFDM_TRY(st.scratch(sizeof(c64) * (size_t)std::max(taps, 1), &dstatic));   // an all-zero h has no taps: H = 0
    OFDM_TRY(txf_static_amps(ch, (c64*)dstatic));
    OFDM_TRY(est_truth(pl, (const c64*)dstatic, 0, dl, genie ? CH : 1, (c64*)dtrue, (double*)dcv));
  }
  ba.errs = (uint32_t*)drows;
  ba.cvals = (const double*)dcv;
  OFDM_TRY(txf_sweep_points(pl, ch, g.points(want_err), nullptr, CH, nullptr, fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    if (fading) OFDM_TRY(est_truth(pl, (const c64*)b.amp, taps, dl, nf, (c64*)dtrue, (double*)dcv));
    EstBodyArgs a = ba;
    a.ref = want_err ? b.ref : nullptr;
    a.inv_snr = 1.0 / std::pow(10.0, g.snr_db[p] * 0.1);                         // MMSE_CE.m:13, the point's own SNR
    const int64_t hs = fading ? (int64_t)nc : 0;
    uint32_t* const ferr = fe.sweep ? fe.at(EST_ROWS * (size_t)at) : nullptr;
    double* const fnm = fn.at(EST_ROWS * (size_t)at);
    EstChunkDone done{nf, p, at, {}, nullptr, nullptr, (const c64*)dtrue, hs, fnm,
                      fading ? (const c64*)b.amp : (const c64*)dstatic, fading ? (int64_t)taps : 0};
    if (pl->f64)
      OFDM_TRY(est_chunk_run<double>(pl, a, b.rx, nf, body, (const c64*)dtrue, hs, fnm, derr + EST_ROWS * p, ferr, dsum + EST_ROWS * p,
                                     ddrop + EST_ROWS * p, done));
    else
      OFDM_TRY(est_chunk_run<float>(pl, a, b.rx, nf, body, (const c64*)dtrue, hs, fnm, derr + EST_ROWS * p, ferr, dsum + EST_ROWS * p,
                                    ddrop + EST_ROWS * p, done));
    return hook ? hook->frames(done) : OFDM_OK;
  }));
  return st.finish();
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_estimator_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                                    int n_taps, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                    int64_t frames_per_point, int64_t frame0, int mmse_mode, int64_t max_frames_per_chunk,
                                    uint64_t* errors_out, double* nmse_sums_out, uint64_t* nmse_dropped_out,
                                    uint32_t* frame_errors_out, double* frame_nmse_out, int flags) {
  const TxfStudyArgs g{h, h_len, tap_delay, tap_power, n_taps, 0, 0, 0, 0.0, nullptr, snr_db, seeds, n_points, frames_per_point, frame0,
                       max_frames_per_chunk, flags};
  return est_study_run(EstStudyCall{pl, g, mmse_mode, errors_out, nmse_sums_out, nmse_dropped_out, frame_errors_out, frame_nmse_out},
                       nullptr);
}
