// The coarse-sync capture: abs(AutoCorr) of AutoCorrFunction(frame, WidthWindow, Nfft) (T4/AutoCorrFunction.m:3-7, plotted at
// T4/Main_model_Task_4.m:282-287) with TgPosition (:10-24) and FreqOffset (:27) of every frame, and the frequency-offset study of
// T4/Main_model_Task_4.m:113-135.
//
//   sync_capture_kernel<T>    one workgroup per frame walks the tiles of acf_tile (sync_core.hpp) in order, every tile from the
//                             same n0 as acf_kernel's, so every rho is bit for bit that of ofdm_AutoCorrFunction.  While a tile's
//                             rho is in LDS: |rho| = sqrt(re^2 + im^2) in double from the stored rho, as acf_plateau_kernel's
//                             predicate forms it, rounded to the plan's precision, goes to the frame's row (coalesced; as double
//                             for the study, where no complex curve reaches HBM), and the search of :10-20 -- first index >
//                             WidthWindow above 0.77 (f), first one not above after it (g), first one above after that (h: a second
//                             run exists) -- advances as the three-state machine of t4_acf_search_kernel, but the walk goes on to
//                             the last tile: the whole curve is wanted.  rho(TgPosition) is picked up when its tile is in LDS (the
//                             tile where g is found, or tile 0 for the catch branch's 65); a plateau that began in an earlier tile
//                             than the one that ends it has that tile formed once more.  Thread 0 ends with the frame's scalars
//                             and, in the study, the two histogram increments (atomics on integers) and the frame's wrapped error.
//   sync_accumulate_kernel    one thread per lag adds: sums[n] = (..(sums[n] + a_0[n]) + a_1[n]) + .. over the chunk's rows in frame
//                             order (the rows staged through LDS by the whole workgroup), a value that is not finite counted in
//                             dropped[n] instead; peak[n] = fmax over the rows.  Its last workgroup adds the chunk's wrapped errors
//                             e in frame order to {sum |e|, sum e^2}.  The chunks of a point run in stream order on accumulators
//                             the call zeroed, so every double is ((0 + v_0) + v_1) + .. whatever the chunking.
// ofdm_sync_study generates each chunk with the fused generator (txf_sweep_points, the RX frames in the plan-owned workspace), runs the
// two kernels on it and never runs a receiver; remove_IFO is out of scope (sync_plan.hpp).  Host side: the checks, the chunk and
// the launch shape are sync_plan.hpp's, plain C++ tested without a GPU.
#include <algorithm>
#include <cmath>

#include "sync_core.hpp"
#include "study_accumulate.hpp"
#include "sync_plan.hpp"
#include "txf_study.hpp"

namespace ofdm {

static_assert(SYNC_ACF_TILE == ACF_TILE && SYNC_ACF_THREADS == ACF_THREADS && SYNC_ACF_MAXW == ACF_MAXW, "sync_plan.hpp restates sync_core.hpp");
static_assert(sizeof(acf4<double>) == 32 && sizeof(acf4<float>) == 16, "sync_plan.hpp restates the prefix table's entry");

// what a frame's workgroup leaves behind; every pointer but tg / fo / status may be null
template <typename T>
struct SyncOut {
  double* rows;              // [frames][n_out] |rho| as double (the study's chunk rows)
  T* amp;                    // [frames][n_out] |rho| (ofdm_rx_acf)
  cx<T>* rho;                // [frames][n_out] (ofdm_rx_acf)
  int64_t* tg;               // [frames] TgPosition, 1-based
  double* fo;                // [frames] FreqOffset
  int32_t* status;           // [frames] 0, or 1: the catch branch (TgPosition 65)
  // the study: the frame's draws (null: 0), the point's tables and the chunk's wrapped errors
  const int64_t* sto;
  const double* cfo;
  unsigned long long *tg_hist, *phase_hist, *fallback;
  double* err;
  int stride;                // Nfft + T_guard
};

// |rho| as acf_plateau_kernel's predicate forms it
template <typename T>
__device__ __forceinline__ double acf_mag(cx<T> v) { return sqrt((double)v.x * v.x + (double)v.y * v.y); }

template <typename T>
__global__ __launch_bounds__(ACF_THREADS) void sync_capture_kernel(const cx<T>* __restrict__ x_all, int64_t len, int W, int nfft,
                                                                   int64_t n_out, double thr, SyncOut<T> o) {
  using acc = acf4<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char acf_smem[];
  acc* const S = (acc*)acf_smem;
  cx<T>* const rt = (cx<T>*)(S + ACF_TILE + W + 1);  // rho of the current tile
  __shared__ acc wtot[ACF_THREADS / 64];
  __shared__ int wmin[ACF_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t fr = blockIdx.x;
  const cx<T>* const x = x_all + fr * len;
  auto tile = [&](int64_t n0) {
    const int n_here = (int)((n_out - n0 < ACF_TILE) ? (n_out - n0) : ACF_TILE);
    acf_tile<T>(x, n0, n_here, W, nfft, S, wtot, [rt](int i, cx<T> r) { rt[i] = r; });
    __syncthreads();
    return n_here;
  };
  // the smallest i in [lo, n_here) of the tile in LDS whose |rho| is above (want_above) / not above the threshold, or -1
  auto first_in_tile = [&](int lo, int n_here, bool want_above) -> int {
    int best = 0x7fffffff;
    for (int i = lo + tid; i < n_here; i += ACF_THREADS) {        // ascending per thread: its first hit is its smallest
      const bool ab = acf_mag(rt[i]) > thr;
      if (ab == want_above) { best = i; break; }
    }
    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
    if (lane == 0) wmin[wid] = best;
    __syncthreads();
    int r = wmin[0];
    for (int w = 1; w < ACF_THREADS / 64; ++w) r = min(r, wmin[w]);
    __syncthreads();
    return r == 0x7fffffff ? -1 : r;
  };
  int stage = 0;                                      // 0: looking for f, 1: g, 2: h, 3: found
  int64_t from = W, f0 = -1, g0 = -1;                 // 1-based index idx = i + 1 must be > W  <=>  i >= W
  bool have = false;                                  // rho(TgPosition) of a found plateau has been read
  double vr = NAN, vi = NAN, r65r = NAN, r65i = NAN;
  int64_t last_n0 = 0;
  for (int64_t n0 = 0; n0 < n_out; n0 += ACF_TILE) {
    const int n_here = tile(n0);
    last_n0 = n0;
    for (int i = tid; i < n_here; i += ACF_THREADS) {
      const cx<T> v = rt[i];
      const T a = (T)acf_mag(v);
      const int64_t at = fr * n_out + n0 + i;
      if (o.rows) o.rows[at] = (double)a;
      if (o.amp) o.amp[at] = a;
      if (o.rho) o.rho[at] = v;
    }
    if (n0 == 0 && n_here > 64) { r65r = (double)rt[64].x; r65i = (double)rt[64].y; }   // AutoCorr(65), the catch branch's
    while (stage < 3) {
      const int lo = from > n0 ? (int)(from - n0) : 0;
      const int r = lo < n_here ? first_in_tile(lo, n_here, stage != 1) : -1;
      if (r < 0) break;
      if (stage == 0) f0 = n0 + r; else if (stage == 1) g0 = n0 + r;
      from = n0 + r + 1;
      ++stage;
    }
    if (stage >= 2 && !have) {
      const int64_t i = ((f0 + 1) + g0) / 2 - 1;      // 0-based TgPosition - 1, should h be found: f0 <= i < g0, g0 is in this tile
      if (i >= n0) { vr = (double)rt[i - n0].x; vi = (double)rt[i - n0].y; have = true; }
    }
    __syncthreads();                                  // the next tile overwrites S and rt
  }
  const int ok = stage == 3;
  const int64_t pos = ok ? ((f0 + 1) + (g0 - 1 + 1)) / 2 : 65;   // :20 floor of the mean of the run's 1-based ends; :23
  if (ok && !have) {                                  // the plateau began in an earlier tile than the one that ends it
    const int64_t pn0 = ((pos - 1) / ACF_TILE) * ACF_TILE;
    if (pn0 != last_n0) tile(pn0);
    vr = (double)rt[pos - 1 - pn0].x; vi = (double)rt[pos - 1 - pn0].y;
  }
  if (!ok) { vr = r65r; vi = r65i; }                  // NaN where the curve has no lag 65 (an index error at :27)
  if (tid == 0) {
    const double fo = -atan2(vi, vr) / (2.0 * M_PI);
    o.tg[fr] = pos;
    o.fo[fr] = fo;
    o.status[fr] = ok ? 0 : 1;
    if (o.tg_hist) {
      if (pos - 1 < n_out) atomicAdd(o.tg_hist + (pos - 1), 1ull);
      if (!ok) atomicAdd(o.fallback, 1ull);
      atomicAdd(o.phase_hist + sync_phase_bin(pos, o.sto ? o.sto[fr] : 0, o.stride), 1ull);
      o.err[fr] = sync_ffo_err(fo, o.cfo ? o.cfo[fr] : 0.0);
    }
  }
}

// rows [nf][n_out] of a chunk into the point's accumulators sums / dropped [n_out] (and peak [n_out]); err [nf] into ffo [2]: the
// column workgroups of study_accumulate.hpp, a value that is not finite dropped, the peak folded over the same rows; the tail
// workgroup adds every wrapped error, finite or not.
__global__ __launch_bounds__(STUDY_ACC_THREADS) void sync_accumulate_kernel(const double* __restrict__ rows, const double* __restrict__ err,
                                                                            int64_t nf, int64_t n_out, double* __restrict__ sums,
                                                                            unsigned long long* __restrict__ dropped,
                                                                            double* __restrict__ peak, double* __restrict__ ffo) {
  __shared__ StudyAccTile tile;
  if (blockIdx.x == gridDim.x - 1) return study_accumulate_scalars<false, false>(tile, err, nullptr, nf, ffo, nullptr);
  study_accumulate_columns<true, ACC_PEAK_ROWS, false>(tile, rows, nullptr, nullptr, nf, n_out, sums, dropped, peak, nullptr);
}

// the capture over nf frames at rx (device memory) in the plan's precision; a launch holds at most 65535 frames
template <typename T>
static int sync_capture_frames(const TxfShape& s, const void* rx, int64_t nf, int W, SyncOut<T> o) {
  const int64_t len = ((int64_t)s.nfft + s.t_guard) * s.n_symb, n_out = sync_n_out(s, W);
  OFDM_HIP(hipFuncSetAttribute((const void*)sync_capture_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sync_capture_lds(sizeof(T) == 8, ACF_MAXW)));
  for (int64_t f0 = 0; f0 < nf; f0 += 65535) {
    const SyncPass p = sync_pass(s, W, std::min<int64_t>(65535, nf - f0));
    if (p.lds != acf_lds_bytes<T>(W) + sizeof(cx<T>) * ACF_TILE || p.lds > SYNC_LDS_LIMIT) {
      set_error("sync_capture_kernel: launch shape differs from the autocorrelation's");
      return OFDM_ERR_STATE;
    }
    SyncOut<T> q = o;
    if (q.rows) q.rows += f0 * n_out;
    if (q.amp) q.amp += f0 * n_out;
    if (q.rho) q.rho += f0 * n_out;
    q.tg += f0; q.fo += f0; q.status += f0;
    if (q.sto) q.sto += f0;
    if (q.cfo) q.cfo += f0;
    if (q.err) q.err += f0;
    hipLaunchKernelGGL(sync_capture_kernel<T>, dim3(p.grid), dim3(p.threads), p.lds, ctx().stream, (const cx<T>*)rx + f0 * len, len, W,
                       s.nfft, n_out, 0.77, q);
    OFDM_TRY(check_launch("sync_capture_kernel"));
  }
  return OFDM_OK;
}

template <typename T>
static int rx_acf_run(const TxfShape& s, const void* rx, int64_t nf, int W, void* amp, void* rho, int64_t* tg, int32_t* status, double* fo) {
  SyncOut<T> o{};
  o.amp = (T*)amp; o.rho = (cx<T>*)rho; o.tg = tg; o.fo = fo; o.status = status;
  o.stride = s.nfft + s.t_guard;
  return sync_capture_frames<T>(s, rx, nf, W, o);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_acf(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int64_t width_window, void* amp_out, void* rho_out,
                           int64_t* tg_position_out, int32_t* status_out, double* freq_offset_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  SyncCapture cap;
  cap.width = width_window;
  cap.out = amp_out || rho_out || tg_position_out || status_out || freq_offset_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(sync_rx_prelude(pl ? &s : nullptr, rx != nullptr, is_f64(flags), n_frames, cap, why), why));
  if (n_frames == 0) return OFDM_OK;
  const int W = (int)width_window;
  const size_t frame_samples = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb, curve = (size_t)sync_n_out(s, W) * (size_t)n_frames;
  Stage st(flags);
  const void* drx;
  void *damp, *drho, *dtg, *dst, *dfo;
  OFDM_TRY(st.in(rx, csize(flags) * frame_samples * (size_t)n_frames, &drx));
  OFDM_TRY(st.out(amp_out, rsize(flags) * curve, &damp));
  OFDM_TRY(st.out(rho_out, csize(flags) * curve, &drho));
  if (tg_position_out) OFDM_TRY(st.out(tg_position_out, sizeof(int64_t) * (size_t)n_frames, &dtg));
  else OFDM_TRY(st.scratch(sizeof(int64_t) * (size_t)n_frames, &dtg));
  if (status_out) OFDM_TRY(st.out(status_out, sizeof(int32_t) * (size_t)n_frames, &dst));
  else OFDM_TRY(st.scratch(sizeof(int32_t) * (size_t)n_frames, &dst));
  if (freq_offset_out) OFDM_TRY(st.out(freq_offset_out, sizeof(double) * (size_t)n_frames, &dfo));
  else OFDM_TRY(st.scratch(sizeof(double) * (size_t)n_frames, &dfo));
  if (pl->f64) OFDM_TRY(rx_acf_run<double>(s, drx, n_frames, W, damp, drho, (int64_t*)dtg, (int32_t*)dst, (double*)dfo));
  else OFDM_TRY(rx_acf_run<float>(s, drx, n_frames, W, damp, drho, (int64_t*)dtg, (int32_t*)dst, (double*)dfo));
  return st.finish();
}

extern "C" int ofdm_sync_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                               int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                               const uint8_t* scr_reg15, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                               int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk, int64_t width_window,
                               double* acf_sums_out, uint64_t* acf_dropped_out, double* acf_peak_out, uint64_t* tg_hist_out,
                               uint64_t* fallback_out, uint64_t* phase_hist_out, double* ffo_err_out, int64_t* frame_tg_out,
                               int32_t* frame_status_out, double* frame_fo_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs a{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  SyncCapture cap;
  cap.width = width_window;
  cap.out = acf_sums_out != nullptr;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(sync_study_prelude(a.call("sync_study", pl ? &s : nullptr), a.both_channels(), cap, ch, fade.gains, why), why));
  const int W = (int)width_window, stride = pl->nfft + pl->t_guard;
  const int64_t n_out = sync_n_out(s, W);
  const size_t np = (size_t)n_points, fpp = (size_t)frames_per_point, no = (size_t)n_out, row = sizeof(double) * no;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  void *dsums, *dpeak;
  TxfFrameOut<int64_t> ftg;
  TxfFrameOut<int32_t> fst;
  TxfFrameOut<double> ffo;
  OFDM_TRY(st.out(acf_sums_out, row * np, &dsums));
  OFDM_TRY(st.out(acf_peak_out, row * np, &dpeak));
  OFDM_TRY(ftg.out(st, frame_tg_out, np * fpp));
  OFDM_TRY(fst.out(st, frame_status_out, np * fpp));
  OFDM_TRY(ffo.out(st, frame_fo_out, np * fpp));
  if (n_points == 0) return st.finish();
  unsigned long long *ddrop, *dtgh, *dfall, *dph;
  double* dferr;
  OFDM_TRY(txf_table(st, acf_dropped_out, no * np, ddrop));
  OFDM_TRY(txf_table(st, tg_hist_out, no * np, dtgh));
  OFDM_TRY(txf_table(st, fallback_out, np, dfall));
  OFDM_TRY(txf_table(st, phase_hist_out, (size_t)stride * np, dph));
  OFDM_TRY(txf_table(st, ffo_err_out, 2 * np, dferr));
  OFDM_HIP(hipMemsetAsync(dsums, 0, row * np, stream));                   // the accumulators: 0 + a_0 + a_1 + ..
  if (dpeak) OFDM_HIP(hipMemsetAsync(dpeak, 0, row * np, stream));
  if (frames_per_point == 0) return st.finish();
  const bool imp_on = a.imp_on();
  const TxfUse u = a.use(ch);
  const int64_t CH = sync_chunk(s, u, frames_per_point, max_frames_per_chunk, W);
  void *rows, *err;
  OFDM_TRY(st.scratch(row * (size_t)CH, &rows));
  OFDM_TRY(st.scratch(sizeof(double) * (size_t)CH, &err));
  OFDM_TRY(ftg.scratch(st, (size_t)CH));
  OFDM_TRY(fst.scratch(st, (size_t)CH));
  OFDM_TRY(ffo.scratch(st, (size_t)CH));
  const TxfImp imp = a.imp();
  OFDM_TRY(txf_sweep_points(pl, ch, a.points(), scr_reg15, CH, imp_on ? &imp : nullptr, a.fading() ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    auto capture = [&](auto zero) {
      using T = decltype(zero);
      SyncOut<T> o{};
      o.rows = (double*)rows; o.tg = ftg.at(at); o.fo = ffo.at(at); o.status = fst.at(at);
      o.sto = imp_on ? b.sto : nullptr; o.cfo = imp_on ? b.cfo : nullptr;
      o.tg_hist = dtgh + no * p;
      o.phase_hist = dph + (size_t)stride * p;
      o.fallback = dfall + p;
      o.err = (double*)err;
      o.stride = stride;
      return sync_capture_frames<T>(s, b.rx, nf, W, o);
    };
    OFDM_TRY(pl->f64 ? capture(0.0) : capture(0.0f));
    const SyncPass sp = sync_pass(s, W, nf);
    hipLaunchKernelGGL(sync_accumulate_kernel, dim3(sp.acc_grid), dim3(sp.acc_threads), 0, stream, (const double*)rows,
                       (const double*)err, nf, n_out, (double*)dsums + no * p, ddrop + no * p,
                       dpeak ? (double*)dpeak + no * p : nullptr, dferr + 2 * p);
    return check_launch("sync_accumulate_kernel");
  }));
  return st.finish();
}
