// The integer-CFO capture: the spectrum remove_IFO thresholds, abs(fft(rx_signal(Nfft+1 : 2*Nfft))) (T4/remove_IFO.m:5), with
// IFO = inds(1) - 1 (:6-8) and the number of bins above 0.77 for every frame, at either of the function's two call sites -- the
// received frame (T4/Main_model_Task_4.m:124-125) or the stream the receiver hands it (T4:278-303) --, and the integer-offset study
// of T4/Main_model_Task_4.m:113-135 (figure 13b of the Task-4 report).
//
//   ifo_capture_kernel<T, N>  one transform (N / 8 threads, the wg_fft of fft_core.hpp, forward, unscaled) per frame.  Slot e of
//                             thread j is sample Nfft + j + e N / 8 of the frame: taken as it is (stage 0), or through the STO fix and
//                             the rotation add_CFO(-FreqOffset) rounded to T (stage 1: t4_raw / t4_rotate of t4_stream.hpp, the
//                             receiver's own bodies), with TgPosition and FreqOffset from the AutoCorrFunction stage that ran in
//                             front.  The spectrum stays in registers: |S(k)| = sqrt(re^2 + im^2) formed in double from the T
//                             spectrum, as first_above_kernel's predicate forms it, is compared with 0.77 there, then rounded to
//                             T and written to the frame's row (as double for the study, with a byte per bin for the
//                             comparison).  The first bin above is a minimum over the thread's eight bins, then over the lanes of
//                             the transform by shuffles and, where a transform spans wavefronts, over those through LDS; the count
//                             of bins above is summed the same way.  Thread 0 of a transform ends with the frame's scalars and, in
//                             the study, the increments of the point's integer tables (atomics on integers) and the frame's total
//                             error.  No complex spectrum and no corrected copy of the frame reaches HBM.
//   ifo_accumulate_kernel     one thread per bin adds: sums[k] = (..(sums[k] + a_0[k]) + a_1[k]) + .. over the chunk's rows in frame
//                             order (the rows staged through LDS by the whole workgroup), a value that is not finite counted in
//                             dropped[k] instead, and counts the frames whose bin k was above.  Its last workgroup adds the
//                             chunk's total errors in frame order to {sum |e|, sum e^2}.  The chunks of a point run in stream order
//                             on accumulators the call zeroed, so every double is ((0 + v_0) + v_1) + .. whatever the chunking.
// ofdm_ifo_study generates each chunk with the fused generator (txf_sweep_points, the RX frames in the plan-owned workspace), runs the
// receiver's AutoCorrFunction stage on it (task4_acf_stage, ofdm_chain_t4.hip) and then the two kernels; no demodulator, no
// equaliser.  Host side: the checks, the chunk and the launch shape are ifo_plan.hpp's, plain C++ tested without a GPU.
#include <algorithm>
#include <cmath>

#include "fft_core.hpp"
#include "ifo_plan.hpp"
#include "study_accumulate.hpp"
#include "t4_stream.hpp"
#include "txf_study.hpp"

namespace ofdm {

// what a frame's transform leaves behind; rows / mask / amp may be null, and the study's block is used where ifo_hist is given
struct IfoOut {
  double* rows;              // [frames][Nfft] |S| as double (the study's chunk rows)
  uint8_t* mask;             // [frames][Nfft] 1 where |S| > 0.77 (the study's chunk rows)
  void* amp;                 // [frames][Nfft] |S| in the plan's precision (ofdm_rx_ifo)
  int32_t *ifo, *status, *n_above;   // [frames]; status holds the AutoCorrFunction stage's on entry
  const int64_t* tg;         // [frames] TgPosition of that stage
  const double* fo;          // [frames] FreqOffset of that stage
  // the study: the frame's Freq_Shift draw (null: 0), the point's tables, the chunk's total errors
  const double* cfo;
  unsigned long long *ifo_hist, *no_line, *err_hist, *err_below, *err_above, *hit, *fallback;
  double* err;
  int64_t span;
};

template <typename T, int N>
__global__ __launch_bounds__(fft_wg_threads(N)) void ifo_capture_kernel(const cx<T>* __restrict__ rx, int64_t len, int64_t n_frames,
                                                                        int sym_len, int stage, int time_desync,
                                                                        const cx<T>* __restrict__ tw, double thr, IfoOut o) {
  constexpr int TPX = N / 8;                          // threads of a transform
  constexpr int XPW = fft_xforms_per_wg(N);
  constexpr int WPX = TPX / 64;                       // wavefronts of a transform (0: several transforms share one)
  constexpr int NONE = 0x7fffffff;
  static_assert(fft_wg_threads(N) / 64 <= IFO_MAX_WAVES, "the search's words per wavefront");
  __shared__ cx<T> lds[XPW * fft_lds_elems(N)];
  __shared__ int32_t wfirst[IFO_MAX_WAVES], wcount[IFO_MAX_WAVES];
  const int g = threadIdx.x / TPX;
  const int j = threadIdx.x % TPX;
  const int64_t f = (int64_t)blockIdx.x * XPW + g;
  const bool live = f < n_frames;                     // a dead transform of the last workgroup still meets every barrier
  const cx<T>* x = rx + (live ? f : 0) * len;
  cx<T> v[8];
  if (!live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = mk<T>(0, 0);
  } else if (stage == IFO_STAGE_RAW) {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = nt_load(x + N + j + e * TPX);
  } else {
    const int64_t pos = time_desync ? o.tg[f] : 0;
    const double cfo = -o.fo[f], inv = 1.0 / (double)N;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = (int64_t)N + j + e * TPX;
      v[e] = t4_rotate<T>(t4_raw<T>(x, i, len, sym_len, time_desync, pos), cfo, i, inv);
    }
  }
  wg_fft<T, N, false>(v, j, tw, lds + g * fft_lds_elems(N));
  int first = NONE, count = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {                       // ascending bins: the first hit is the thread's smallest
    const int k = j + e * TPX;
    const double m = sqrt((double)v[e].x * v[e].x + (double)v[e].y * v[e].y);
    const bool above = m > thr;
    if (above && first == NONE) first = k;
    count += above ? 1 : 0;
    if (live) {
      const T a = (T)m;
      const int64_t at = f * N + k;
      if (o.rows) o.rows[at] = (double)a;
      if (o.mask) o.mask[at] = above ? 1 : 0;
      if (o.amp) ((T*)o.amp)[at] = a;
    }
  }
  // over the lanes of the transform: aligned groups of TPX lanes below a wavefront, else the whole wavefront
#pragma unroll
  for (int off = (TPX < 64 ? TPX : 64) / 2; off > 0; off >>= 1) {
    first = min(first, __shfl_xor(first, off, 64));
    count += __shfl_xor(count, off, 64);
  }
  if constexpr (WPX > 1) {                            // over the wavefronts of the transform
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { wfirst[wave] = first; wcount[wave] = count; }
    __syncthreads();
    if (j == 0) {
      first = NONE; count = 0;
      for (int w = g * WPX; w < (g + 1) * WPX; ++w) { first = min(first, wfirst[w]); count += wcount[w]; }
    }
  }
  if (j != 0 || !live) return;
  const bool line = first != NONE;
  const int32_t ifo = line ? first : 0;
  int32_t st = o.status[f];
  if (!line && st >= 0) st = -1;                      // no bin above: the script stops at inds(1); the receiver marks the frame
  o.ifo[f] = ifo;
  o.status[f] = st;
  o.n_above[f] = count;
  if (!o.ifo_hist) return;
  if (st == 1) atomicAdd(o.fallback, 1ull);
  if (!line) {
    atomicAdd(o.no_line, 1ull);
    o.err[f] = NAN;                                   // left out of the sums
    return;
  }
  atomicAdd(o.ifo_hist + ifo, 1ull);
  const double draw = o.cfo ? o.cfo[f] : 0.0;
  const int b = ifo_err_bin(ifo, draw, o.span);
  atomicAdd(b >= 0 ? o.err_hist + b : b == IFO_ERR_BELOW ? o.err_below : o.err_above, 1ull);
  if (b == (int)o.span) atomicAdd(o.hit, 1ull);
  o.err[f] = cfo_total_err(o.fo[f], ifo, draw);
}

// rows / mask [nf][nfft] of a chunk into the point's sums / dropped / above_counts [nfft]; err [nf] into cfo_err [2]: the column
// workgroups of study_accumulate.hpp, a value that is not finite dropped, the mask bytes counted; the tail workgroup takes the
// column of total errors, a frame without a line (NaN) left out.
__global__ __launch_bounds__(STUDY_ACC_THREADS) void ifo_accumulate_kernel(const double* __restrict__ rows, const uint8_t* __restrict__ mask,
                                                                           const double* __restrict__ err, int64_t nf, int nfft,
                                                                           double* __restrict__ sums, unsigned long long* __restrict__ dropped,
                                                                           unsigned long long* __restrict__ above_counts,
                                                                           double* __restrict__ cfo_err) {
  __shared__ StudyAccTile tile;
  if (blockIdx.x == gridDim.x - 1) return study_accumulate_scalars<true, false>(tile, err, nullptr, nf, cfo_err, nullptr);
  study_accumulate_columns<true, ACC_PEAK_OFF, true>(tile, rows, nullptr, mask, nf, nfft, sums, dropped, nullptr, above_counts);
}

template <typename T, int N>
static int launch_ifo_capture(const IfoPass& p, const void* rx, int64_t len, int64_t nf, int sym_len, int stage, int time_desync,
                              const void* tw, const IfoOut& o) {
  static_assert(fft_wg_threads(N) == ifo_threads(N) && fft_xforms_per_wg(N) == ifo_frames_per_wg(N), "ifo_plan.hpp restates fft_core.hpp");
  if (p.threads != fft_wg_threads(N) || p.frames_per_wg != fft_xforms_per_wg(N) ||
      p.lds != sizeof(cx<T>) * (size_t)fft_xforms_per_wg(N) * fft_lds_elems(N) + 2 * sizeof(int32_t) * IFO_MAX_WAVES || p.lds > SYNC_LDS_LIMIT) {
    set_error("ifo_capture_kernel: launch shape differs from the transform's");
    return OFDM_ERR_STATE;
  }
  hipLaunchKernelGGL((ifo_capture_kernel<T, N>), dim3(p.grid), dim3(p.threads), 0, ctx().stream, (const cx<T>*)rx, len, nf, sym_len,
                     stage, time_desync, (const cx<T>*)tw, 0.77, o);
  return check_launch("ifo_capture_kernel");
}

// the capture over nf frames at rx (device memory) in the plan's precision and Nfft; o.tg / o.fo / o.status hold the
// AutoCorrFunction stage's results
static int ifo_capture_frames(const ofdm_rx_plan* pl, const TxfShape& s, const void* rx, int64_t nf, int stage, int time_desync,
                              const IfoOut& o) {
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &tw));
  const IfoPass p = ifo_pass(s, nf);
  const int sym_len = pl->nfft + pl->t_guard;
  const int64_t len = (int64_t)sym_len * pl->n_symb;
#define CALL(NN)                                                                                                   \
  if (pl->f64) OFDM_TRY((launch_ifo_capture<double, NN>(p, rx, len, nf, sym_len, stage, time_desync, tw, o)));    \
  else OFDM_TRY((launch_ifo_capture<float, NN>(p, rx, len, nf, sym_len, stage, time_desync, tw, o)));
  OFDM_FFT_DISPATCH(pl->nfft, CALL)
#undef CALL
  return OFDM_OK;
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_ifo(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int stage, int time_desync, void* amp_out,
                           int32_t* ifo_out, int32_t* status_out, int32_t* n_above_out, int64_t* tg_position_out,
                           double* freq_offset_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  IfoCapture cap;
  cap.stage = stage;
  cap.time_desync = time_desync;
  cap.out = amp_out || ifo_out || status_out || n_above_out || tg_position_out || freq_offset_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(ifo_rx_prelude(pl ? &s : nullptr, rx != nullptr, is_f64(flags), n_frames, cap, why), why));
  if (n_frames == 0) return OFDM_OK;
  const size_t nf = (size_t)n_frames, N = (size_t)pl->nfft, frame_samples = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  Stage st(flags);
  const void* drx;
  void *damp, *difo, *dst, *dna, *dtg, *dfo;
  OFDM_TRY(st.in(rx, csize(flags) * frame_samples * nf, &drx));
  OFDM_TRY(st.out(amp_out, rsize(flags) * N * nf, &damp));
  // the scalars are always produced (scratch when the caller does not want them)
  auto scalar = [&st](void* user, size_t bytes, void** d) { return user ? st.out(user, bytes, d) : st.scratch(bytes, d); };
  OFDM_TRY(scalar(ifo_out, sizeof(int32_t) * nf, &difo));
  OFDM_TRY(scalar(status_out, sizeof(int32_t) * nf, &dst));
  OFDM_TRY(scalar(n_above_out, sizeof(int32_t) * nf, &dna));
  OFDM_TRY(scalar(tg_position_out, sizeof(int64_t) * nf, &dtg));
  OFDM_TRY(scalar(freq_offset_out, sizeof(double) * nf, &dfo));
  for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {                       // a launch of the stage in front holds at most 65535
    const int64_t n = std::min<int64_t>(65535, n_frames - f0);
    const void* const x = (const unsigned char*)drx + csize(flags) * frame_samples * (size_t)f0;
    IfoOut o{};
    o.amp = damp ? (unsigned char*)damp + rsize(flags) * N * (size_t)f0 : nullptr;
    o.ifo = (int32_t*)difo + f0; o.status = (int32_t*)dst + f0; o.n_above = (int32_t*)dna + f0;
    int64_t* const tg = (int64_t*)dtg + f0;
    double* const fo = (double*)dfo + f0;
    o.tg = tg; o.fo = fo;
    OFDM_TRY(task4_acf_stage(pl, x, n, time_desync, tg, fo, o.ifo, o.status));
    OFDM_TRY(ifo_capture_frames(pl, s, x, n, stage, time_desync, o));
  }
  return st.finish();
}

extern "C" int ofdm_ifo_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                              int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int stage,
                              int time_desync, const uint8_t* scr_reg15, const double* snr_db, const uint64_t* seeds,
                              int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                              int64_t err_span, double* spec_sums_out, uint64_t* spec_dropped_out, uint64_t* above_counts_out,
                              uint64_t* ifo_hist_out, uint64_t* no_line_out, uint64_t* err_hist_out, uint64_t* err_below_out,
                              uint64_t* err_above_out, uint64_t* hit_out, double* cfo_err_out, uint64_t* fallback_out,
                              int32_t* frame_ifo_out, int32_t* frame_status_out, int32_t* frame_n_above_out, int64_t* frame_tg_out,
                              double* frame_fo_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs a{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  IfoCapture cap;
  cap.stage = stage;
  cap.time_desync = time_desync;
  cap.study = true;
  cap.err_span = err_span;
  cap.out = spec_sums_out || spec_dropped_out || above_counts_out || ifo_hist_out || no_line_out || err_hist_out || err_below_out ||
            err_above_out || hit_out || cfo_err_out || fallback_out || frame_ifo_out || frame_status_out || frame_n_above_out ||
            frame_tg_out || frame_fo_out;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(ifo_study_prelude(a.call("ifo_study", pl ? &s : nullptr), a.both_channels(), cap, ch, fade.gains, why), why));
  const size_t N = (size_t)pl->nfft, np = (size_t)n_points, fpp = (size_t)frames_per_point, nerr = 2 * (size_t)err_span + 1;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  TxfFrameOut<int32_t> fifo, fst, fna;
  TxfFrameOut<int64_t> ftg;
  TxfFrameOut<double> ffo;
  OFDM_TRY(fifo.out(st, frame_ifo_out, np * fpp));
  OFDM_TRY(fst.out(st, frame_status_out, np * fpp));
  OFDM_TRY(fna.out(st, frame_n_above_out, np * fpp));
  OFDM_TRY(ftg.out(st, frame_tg_out, np * fpp));
  OFDM_TRY(ffo.out(st, frame_fo_out, np * fpp));
  if (n_points == 0) return st.finish();
  double *dsums, *dcerr;
  unsigned long long *ddrop, *dabove, *dhist, *dnone, *dehist, *debelow, *deabove, *dhit, *dfall;
  OFDM_TRY(txf_table(st, spec_sums_out, N * np, dsums));
  OFDM_TRY(txf_table(st, spec_dropped_out, N * np, ddrop));
  OFDM_TRY(txf_table(st, above_counts_out, N * np, dabove));
  OFDM_TRY(txf_table(st, ifo_hist_out, N * np, dhist));
  OFDM_TRY(txf_table(st, no_line_out, np, dnone));
  OFDM_TRY(txf_table(st, err_hist_out, nerr * np, dehist));
  OFDM_TRY(txf_table(st, err_below_out, np, debelow));
  OFDM_TRY(txf_table(st, err_above_out, np, deabove));
  OFDM_TRY(txf_table(st, hit_out, np, dhit));
  OFDM_TRY(txf_table(st, cfo_err_out, 2 * np, dcerr));
  OFDM_TRY(txf_table(st, fallback_out, np, dfall));
  if (frames_per_point == 0) return st.finish();
  const bool imp_on = a.imp_on();
  const TxfUse u = a.use(ch);
  const int64_t CH = ifo_chunk(s, u, frames_per_point, max_frames_per_chunk);
  const size_t chn = (size_t)CH;
  void *rows, *mask, *err;
  OFDM_TRY(st.scratch(sizeof(double) * N * chn, &rows));
  OFDM_TRY(st.scratch(N * chn, &mask));
  OFDM_TRY(st.scratch(sizeof(double) * chn, &err));
  OFDM_TRY(fifo.scratch(st, chn));
  OFDM_TRY(fst.scratch(st, chn));
  OFDM_TRY(fna.scratch(st, chn));
  OFDM_TRY(ftg.scratch(st, chn));
  OFDM_TRY(ffo.scratch(st, chn));
  const IfoPass ip = ifo_pass(s, CH);
  const TxfImp imp = a.imp();
  OFDM_TRY(txf_sweep_points(pl, ch, a.points(), scr_reg15, CH, imp_on ? &imp : nullptr, a.fading() ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    IfoOut o{};
    o.rows = (double*)rows; o.mask = (uint8_t*)mask;
    o.ifo = fifo.at(at); o.status = fst.at(at); o.n_above = fna.at(at);
    int64_t* const tg = ftg.at(at);
    double* const fo = ffo.at(at);
    o.tg = tg; o.fo = fo;
    o.cfo = imp_on ? b.cfo : nullptr;
    o.ifo_hist = dhist + N * p; o.no_line = dnone + p; o.err_hist = dehist + nerr * p; o.err_below = debelow + p;
    o.err_above = deabove + p; o.hit = dhit + p; o.fallback = dfall + p;
    o.err = (double*)err;
    o.span = err_span;
    OFDM_TRY(task4_acf_stage(pl, b.rx, nf, time_desync, tg, fo, o.ifo, o.status));
    OFDM_TRY(ifo_capture_frames(pl, s, b.rx, nf, stage, time_desync, o));
    hipLaunchKernelGGL(ifo_accumulate_kernel, dim3(ip.acc_grid), dim3(ip.acc_threads), 0, stream, (const double*)rows,
                       (const uint8_t*)mask, (const double*)err, nf, pl->nfft, dsums + N * p, ddrop + N * p, dabove + N * p,
                       dcerr + 2 * p);
    return check_launch("ifo_accumulate_kernel");
  }));
  return st.finish();
}
