// The received-spectrum capture: abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard))) of T3/Main_model_Task_3.m:138 and
// T5/Main_model_Task_5.m:131, the useful part of symbol 2 at T4/Main_model_Task_4.m:268, and -- on a clean stream -- the
// abs(RX_OFDM_mapped_carriers(:,1)) of T1/Main_model.m:77.
//
//   spectrum_kernel<T, N>        one transform (N / 8 threads, the wg_fft of fft_core.hpp, forward, unscaled) per frame; window
//                                w = 0 .. n_windows - 1 is the frame's samples first + w (N + T_guard) .. + N - 1.  Per window
//                                amp[f][w][k] = |S(k)| in T; per frame power[f][k] = sum_w (re^2 + im^2) in double, re and im
//                                widened before squaring, the sum taken by the bin's own thread in window order (no atomics), and
//                                peak[f][k] = the fmax of the same terms.  Every load is one complex sample wide (8 bytes in
//                                float, 16 in double) at an address that is a multiple of that for any `first`; nothing wider is
//                                formed, so an odd `first` needs no second path.  Slot e of thread j is sample j + e N / 8:
//                                consecutive lanes read and write consecutive elements.
//   spectrum_accumulate_kernel   one thread per bin adds: sums[k] = (..(sums[k] + P_0[k]) + P_1[k]) + .. over the chunk's rows in frame
//                                order (the rows staged through LDS by the whole workgroup), peak[k] = fmax over them.  The chunks of a point run in stream order on the accumulators
//                                the call zeroed, so the result is ((0 + P_0) + P_1) + .. whatever the chunking.
// ofdm_spectrum_study generates each chunk with the fused generator (the studies' scaffold, txf_study.hpp: the RX frames in the
// plan-owned workspace), runs the two kernels on it and never runs a receiver.  Host side: the checks, the chunk and the launch
// shape are spectrum_plan.hpp's, plain C++ tested without a GPU.
#include <algorithm>
#include <cmath>

#include "fft_core.hpp"
#include "spectrum_plan.hpp"
#include "study_accumulate.hpp"
#include "txf_study.hpp"

namespace ofdm {

// rx: frames of frame_samples; window w of frame f starts at rx + f * frame_samples + first + w * stride
// amp (optional) [n_frames][n_windows][N]; power (optional) [n_frames][N]; peak (optional) [n_frames][N]
template <typename T, int N>
__global__ __launch_bounds__(fft_wg_threads(N)) void spectrum_kernel(const cx<T>* __restrict__ rx, int64_t frame_samples,
                                                                     int64_t n_frames, int64_t first, int stride,
                                                                     int64_t n_windows, const cx<T>* __restrict__ tw,
                                                                     T* __restrict__ amp, double* __restrict__ power,
                                                                     double* __restrict__ peak) {
  constexpr int TPX = N / 8;
  constexpr int XPW = fft_xforms_per_wg(N);
  __shared__ cx<T> lds[XPW * fft_lds_elems(N)];
  const int g = threadIdx.x / TPX;
  const int j = threadIdx.x % TPX;
  const int64_t f = (int64_t)blockIdx.x * XPW + g;
  const bool live = f < n_frames;                     // a dead transform of the last workgroup still meets every barrier
  const cx<T>* x = rx + (live ? f : 0) * frame_samples + first;
  double pw[8], pk[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) pw[e] = pk[e] = 0.0;
  for (int64_t w = 0; w < n_windows; ++w) {
    cx<T> v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = live ? x[w * stride + j + e * TPX] : mk<T>(0, 0);
    wg_fft<T, N, false>(v, j, tw, lds + g * fft_lds_elems(N));
    if (live) {
      T* a = amp ? amp + (f * n_windows + w) * N : nullptr;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (a) a[j + e * TPX] = sqrt(v[e].x * v[e].x + v[e].y * v[e].y);
        const double re = (double)v[e].x, im = (double)v[e].y;
        const double p = re * re + im * im;
        pw[e] += p;
        pk[e] = fmax(pk[e], p);
      }
    }
  }
  if (live) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (power) power[f * N + j + e * TPX] = pw[e];
      if (peak) peak[f * N + j + e * TPX] = pk[e];
    }
  }
}

// rows [nf][nfft] (and peak_rows, optional) of a chunk into the point's accumulators sums [nfft] (and peak [nfft]): the column
// workgroups of study_accumulate.hpp, every value added, the peak folded over peak_rows; no scalars, so no tail workgroup.
__global__ __launch_bounds__(STUDY_ACC_THREADS) void spectrum_accumulate_kernel(const double* __restrict__ rows,
                                                                                const double* __restrict__ peak_rows, int64_t nf,
                                                                                int nfft, double* __restrict__ sums,
                                                                                double* __restrict__ peak) {
  __shared__ StudyAccTile tile;
  study_accumulate_columns<false, ACC_PEAK_SECOND, false>(tile, rows, peak_rows, nullptr, nf, nfft, sums, nullptr, peak, nullptr);
}

template <typename T, int N>
static int launch_spectrum(const SpecPass& p, const void* rx, int64_t frame_samples, int64_t nf, int64_t first, int stride,
                           int64_t n_windows, const void* tw, void* amp, double* power, double* peak) {
  static_assert(fft_wg_threads(N) == (N / 8 > 256 ? N / 8 : 256), "spectrum_plan.hpp restates fft_wg_threads");
  if (p.threads != fft_wg_threads(N) || p.frames_per_wg != fft_xforms_per_wg(N) ||
      p.lds != sizeof(cx<T>) * (size_t)fft_xforms_per_wg(N) * fft_lds_elems(N)) {
    set_error("spectrum_kernel: launch shape differs from the transform's");
    return OFDM_ERR_STATE;
  }
  hipLaunchKernelGGL((spectrum_kernel<T, N>), dim3(p.grid), dim3(p.threads), 0, ctx().stream, (const cx<T>*)rx, frame_samples, nf,
                     first, stride, n_windows, (const cx<T>*)tw, (T*)amp, power, peak);
  return check_launch("spectrum_kernel");
}

// the spectrum pass over nf frames at rx (device memory) in the plan's precision and Nfft
static int spectrum_frames(const ofdm_rx_plan* pl, const TxfShape& s, const void* rx, int64_t nf, int64_t first, int64_t n_windows,
                           void* amp, double* power, double* peak) {
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &tw));
  const SpecPass p = spectrum_pass(s, nf);
  const int stride = pl->nfft + pl->t_guard;
  const int64_t fs = (int64_t)stride * pl->n_symb;
#define CALL(NN)                                                                                                  \
  if (pl->f64) OFDM_TRY((launch_spectrum<double, NN>(p, rx, fs, nf, first, stride, n_windows, tw, amp, power, peak))); \
  else OFDM_TRY((launch_spectrum<float, NN>(p, rx, fs, nf, first, stride, n_windows, tw, amp, power, peak)));
  OFDM_FFT_DISPATCH(pl->nfft, CALL)
#undef CALL
  return OFDM_OK;
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_spectrum(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int64_t first, int64_t n_windows,
                                void* amp_out, double* power_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  SpecCapture cap;
  cap.first = first; cap.n_windows = n_windows; cap.out = amp_out || power_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(spectrum_rx_prelude(pl ? &s : nullptr, rx != nullptr, is_f64(flags), n_frames, cap, why), why));
  if (n_frames == 0) return OFDM_OK;
  const int64_t frame_samples = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  Stage st(flags);
  const void* drx;
  void *damp, *dpow;
  OFDM_TRY(st.in(rx, csize(flags) * (size_t)frame_samples * n_frames, &drx));
  OFDM_TRY(st.out(amp_out, rsize(flags) * (size_t)pl->nfft * n_windows * n_frames, &damp));
  OFDM_TRY(st.out(power_out, sizeof(double) * (size_t)pl->nfft * n_frames, &dpow));
  OFDM_TRY(spectrum_frames(pl, s, drx, n_frames, first, n_windows, damp, (double*)dpow, nullptr));
  return st.finish();
}

extern "C" int ofdm_spectrum_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                                   int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                                   const uint8_t* scr_reg15, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                   int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk, int64_t first,
                                   int64_t n_windows, double* power_sums_out, double* power_peak_out, double* frame_power_out,
                                   int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs a{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  SpecCapture cap;
  cap.first = first; cap.n_windows = n_windows; cap.out = power_sums_out != nullptr;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(spectrum_study_prelude(a.call("spectrum_study", pl ? &s : nullptr), a.both_channels(), cap, ch, fade.gains, why), why));
  const size_t nfft = (size_t)pl->nfft, row = sizeof(double) * nfft, np = (size_t)n_points;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  void *dsums, *dpeak;
  TxfFrameOut<double> fp;
  OFDM_TRY(st.out(power_sums_out, row * np, &dsums));
  OFDM_TRY(st.out(power_peak_out, row * np, &dpeak));
  OFDM_TRY(fp.out(st, frame_power_out, nfft * np * (size_t)frames_per_point));
  if (n_points == 0) return st.finish();
  OFDM_HIP(hipMemsetAsync(dsums, 0, row * np, stream));                   // the accumulators: 0 + P_0 + P_1 + ..
  if (dpeak) OFDM_HIP(hipMemsetAsync(dpeak, 0, row * np, stream));
  if (frames_per_point == 0) return st.finish();
  const TxfUse u = a.use(ch);
  const int64_t CH = spectrum_chunk(s, u, frames_per_point, max_frames_per_chunk, dpeak != nullptr);
  void* peak_rows = nullptr;
  OFDM_TRY(fp.scratch(st, nfft * (size_t)CH));
  if (dpeak) OFDM_TRY(st.scratch(row * (size_t)CH, &peak_rows));
  const TxfImp imp = a.imp();
  OFDM_TRY(txf_sweep_points(pl, ch, a.points(), scr_reg15, CH, a.imp_on() ? &imp : nullptr, a.fading() ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    double* const pr = fp.at(nfft * (size_t)at);
    OFDM_TRY(spectrum_frames(pl, s, b.rx, nf, first, n_windows, nullptr, pr, (double*)peak_rows));
    const SpecPass sp = spectrum_pass(s, nf);
    hipLaunchKernelGGL(spectrum_accumulate_kernel, dim3(sp.acc_grid), dim3(sp.acc_threads), 0, stream, (const double*)pr,
                       (const double*)peak_rows, nf, (int)nfft, (double*)dsums + nfft * (size_t)p,
                       dpeak ? (double*)dpeak + nfft * (size_t)p : nullptr);
    return check_launch("spectrum_accumulate_kernel");
  }));
  return st.finish();
}
