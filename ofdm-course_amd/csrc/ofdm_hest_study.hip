// The channel-estimate capture: the two outputs of estimate_channel (T4/estimate_channel.m:6,:8) -- Hest_at_pilots and H_est -- of
// every frame behind the receiver's front end and fine_sync, and the channel study of figure 21 of the Task-4 report
// (T4/Main_model_Task_4.m:318-332): |H_est|, |H| and the stems |Hest_at_pilots| over the carrier index, with the error of the
// estimate against the frame's true channel per carrier, per pilot and per frame.
//
//   hest_static_table_kernel  a static channel's H(k) on carriers 1..N_carrier, once per call (channel_resp, channel_resp.hpp).
//   hest_capture_kernel<T>    the chunk's rows.  Workgroups of 256 threads cover whole frames with the carriers across the lanes
//                             (below 256 carriers several frames per workgroup: hest_plan.hpp), so the loads of H_est and the
//                             stores of the rows are coalesced; the frame's taps are staged once in LDS (a channel per frame) or
//                             H comes from the table (static).  Per carrier four doubles -- |H_est|, |H|, |H - H_est|^2,
//                             (|H_est| - |H|)^2 -- and a byte "H_est is not finite"; per pilot |Hest_at_pilots|,
//                             |H(pilotCarriers(i)) - Hest_at_pilots(i)|^2 and the byte.  |z| = sqrt(re re + im im) in double,
//                             the two products and the sum rounded one by one.
//   hest_frame_sum_kernel     sum_k (|H_est| - |H|)^2 of a frame in the order of t5_frame_nmse_kernel: a stride of 256 per
//                             thread, the butterfly of a wavefront, the four wave partials paired.
//   hest_accumulate_kernel    one thread per carrier (pilot) and quantity adds the chunk's rows in frame order (staged through LDS
//                             by the whole workgroup); a frame whose byte is set adds nothing and is counted in dropped.  The
//                             chunks of a point run in stream order on accumulators the call zeroed, so every double is
//                             ((0 + v_0) + v_1) + .. whatever the chunking.
//   hest_thresholds_kernel    the host's table of linear thresholds into device memory (kernel arguments, no host wait).
//   hest_frame_hist_kernel    after the last chunk: every frame's error sum binned on the table of linear thresholds (hest_bin,
//                             hest_plan.hpp) and its status counted (atomics on integers).
// ofdm_hest_study generates each chunk with the fused generator (txf_sweep_points), runs the receiver up to and including
// estimate_channel on it (task4_estimate, ofdm_chain_t4.hip), the sweeps' own error kernel on the arena's H (txf_frame_nmse) and
// the kernels above; no equaliser, no demapper.  Host side: the checks, the chunk and the launch shape are hest_plan.hpp's.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hest_plan.hpp"
#include "hest_point.hpp"
#include "txf_study.hpp"

namespace ofdm {

// the rows of a chunk: car [frames][4][N_carrier], cmask [frames][N_carrier], pil [frames][2][Np], pmask [frames][Np]
struct HestRows {
  double* car;
  uint8_t* cmask;
  double* pil;
  uint8_t* pmask;
};

__global__ __launch_bounds__(256) void hest_static_table_kernel(const c64* __restrict__ amp, TxfDelays dl, int nfft, int n_carrier,
                                                                c64* __restrict__ htab) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n_carrier) return;
  double hr, hi;
  channel_resp(amp, dl, k, nfft, 2.0 / (double)nfft, hr, hi);
  htab[k] = mk<double>(hr, hi);
}

template <typename T>
__global__ __launch_bounds__(HEST_THREADS) void hest_capture_kernel(const cx<T>* __restrict__ hest, const cx<T>* __restrict__ hp,
                                                                    const int32_t* __restrict__ pc0, const c64* __restrict__ amp,
                                                                    int64_t amp_stride, TxfDelays dl, const c64* __restrict__ htab,
                                                                    int nfft, int n_carrier, int np, int lanes, int64_t n_frames,
                                                                    HestRows o) {
  __shared__ c64 taps[HEST_MAX_FRAMES_PER_WG * TXF_MAX_TAPS];
  const int per = HEST_THREADS / lanes;
  const int g = threadIdx.x / lanes, j = threadIdx.x % lanes;
  const int64_t f = (int64_t)blockIdx.x * per + g;
  const bool live = f < n_frames;                     // a dead frame of the last workgroup still meets the barrier
  c64* const a = taps + g * TXF_MAX_TAPS;
  if (!htab) {                                        // a channel per frame: its taps once, for every carrier and pilot
    if (live)
      for (int t = j; t < dl.n; t += lanes) a[t] = amp[f * amp_stride + t];
    __syncthreads();
  }
  if (!live) return;
  const double inv = 2.0 / (double)nfft;
  double* const car = o.car + f * (int64_t)HEST_CARRIER_ROWS * n_carrier;
  for (int k = j; k < n_carrier; k += lanes) {
    double hr, hi;
    if (htab) { const c64 h = htab[k]; hr = h.x; hi = h.y; }
    else channel_resp(a, dl, k, nfft, inv, hr, hi);
    const HestPoint p = hest_point<T>(hr, hi, hest[f * n_carrier + k]);
    car[k] = p.est_amp;
    car[n_carrier + k] = p.true_amp;
    car[2 * n_carrier + k] = p.err;
    car[3 * n_carrier + k] = p.amp_err;
    o.cmask[f * n_carrier + k] = p.bad;
  }
  double* const pil = o.pil + f * (int64_t)HEST_PILOT_ROWS * np;
  for (int i = j; i < np; i += lanes) {
    const int k = pc0[i];                             // 0-based carrier of pilot i, inside 0 .. N_carrier - 1
    double hr, hi;
    if (htab) { const c64 h = htab[k]; hr = h.x; hi = h.y; }
    else channel_resp(a, dl, k, nfft, inv, hr, hi);
    const HestPoint p = hest_point<T>(hr, hi, hp[f * np + i]);
    pil[i] = p.est_amp;
    pil[np + i] = p.err;
    o.pmask[f * np + i] = p.bad;
  }
}

// out[f] = sum_k car[f][3][k], the order of t5_frame_nmse_kernel; a value that is not finite passes into the sum
__global__ __launch_bounds__(256) void hest_frame_sum_kernel(const double* __restrict__ car, int n_carrier, double* __restrict__ out) {
  __shared__ double part[4];
  const int64_t f = blockIdx.x;
  const double* const row = car + (f * (int64_t)HEST_CARRIER_ROWS + 3) * n_carrier;
  double s = 0;
  for (int k = threadIdx.x; k < n_carrier; k += 256) s += row[k];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[f] = (part[0] + part[1]) + (part[2] + part[3]);
}

// the accumulators of one point: quantity q of column k at sums[q][k]
struct HestSums {
  double* sums[HEST_CARRIER_ROWS];
  unsigned long long* dropped;
};

// rows [nf][nq][ncols] and mask [nf][ncols] of a chunk into the point's sums [nq][ncols] and dropped [ncols].  A workgroup owns
// STUDY_ACC_COLS columns of quantity blockIdx.y.  The sum of a column is one chain of additions, so the loads are what can overlap:
// the four wavefronts stage STUDY_ACC_TILE rows at a time in LDS, then wavefront 0 adds the tile to its columns in frame order.
// Its own body, not study_accumulate.hpp's: the exclusion is a mask byte staged beside the double, and the quantities are blockIdx.y.
__global__ __launch_bounds__(STUDY_ACC_THREADS) void hest_accumulate_kernel(const double* __restrict__ rows, const uint8_t* __restrict__ mask,
                                                                           int64_t nf, int nq, int ncols, HestSums acc) {
  __shared__ double tile[STUDY_ACC_TILE][STUDY_ACC_COLS];
  __shared__ uint8_t bad[STUDY_ACC_TILE][STUDY_ACC_COLS];
  constexpr int RW = STUDY_ACC_THREADS / STUDY_ACC_COLS;                       // row groups: 4
  constexpr int PER = STUDY_ACC_TILE / RW;                                    // rows per thread and tile
  const int q = blockIdx.y;
  const int c = threadIdx.x % STUDY_ACC_COLS, r = threadIdx.x / STUDY_ACC_COLS;
  const int k = blockIdx.x * STUDY_ACC_COLS + c;
  const bool col = k < ncols;                                                // the last workgroup's columns past the end
  double* const sums = acc.sums[q];
  double s = (r == 0 && col) ? sums[k] : 0.0;
  unsigned long long nd = 0;
  for (int64_t t0 = 0; t0 < nf; t0 += STUDY_ACC_TILE) {
    double v[PER];
    uint8_t m[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int64_t f = t0 + r * PER + i;
      const bool in = col && f < nf;
      v[i] = in ? rows[(f * nq + q) * ncols + k] : 0.0;
      m[i] = in ? mask[f * ncols + k] : (uint8_t)0;
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) { tile[r * PER + i][c] = v[i]; bad[r * PER + i][c] = m[i]; }
    __syncthreads();
    if (r == 0) {
      const int n = (int)(nf - t0 < STUDY_ACC_TILE ? nf - t0 : STUDY_ACC_TILE);
      // sixteen rows into registers at a time (independent LDS reads), then the chain on them -- the same additions in the same
      // order; a row that is left out is a select, not a branch (its sum, maybe NaN, is discarded).  The rest one by one.
      int i0 = 0;
      for (; i0 + 16 <= n; i0 += 16) {
        double tv[16];
        uint8_t tm[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { tv[i] = tile[i0 + i][c]; tm[i] = bad[i0 + i][c]; }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const double t = s + tv[i];
          s = tm[i] ? s : t;
          nd += tm[i] ? 1ull : 0ull;
        }
      }
      for (int i = i0; i < n; ++i) {
        if (bad[i][c]) ++nd;
        else s += tile[i][c];
      }
    }
    __syncthreads();
  }
  if (r == 0 && col) {
    sums[k] = s;
    if (q == 0) acc.dropped[k] += nd;
  }
}

// the host's table of thresholds into device memory, HEST_THR_PART entries per launch (kernel arguments: no copy the host waits for)
constexpr int HEST_THR_PART = 256;
struct HestThrPart {
  double v[HEST_THR_PART];
};

__global__ __launch_bounds__(HEST_THR_PART) void hest_thresholds_kernel(double* __restrict__ thr, HestThrPart part, int n) {
  if ((int)threadIdx.x < n) thr[threadIdx.x] = part.v[threadIdx.x];
}

int study_thresholds_device(const double* thr, size_t n, double* dthr) {
  for (size_t i0 = 0; i0 < n; i0 += HEST_THR_PART) {
    const int m = (int)std::min<size_t>(HEST_THR_PART, n - i0);
    HestThrPart part{};
    std::copy(thr + i0, thr + i0 + m, part.v);
    hipLaunchKernelGGL(hest_thresholds_kernel, dim3(1), dim3(HEST_THR_PART), 0, ctx().stream, dthr + i0, part, m);
  }
  return check_launch("hest_thresholds_kernel");
}

// every frame of the sweep: its error sum on the table of thresholds, its status
__global__ __launch_bounds__(256) void hest_frame_hist_kernel(const double* __restrict__ frame_nmse, const int32_t* __restrict__ status,
                                                              int64_t frames_per_point, int64_t n_total, const double* __restrict__ thr,
                                                              int n_bins, unsigned long long* __restrict__ hist,
                                                              unsigned long long* __restrict__ below, unsigned long long* __restrict__ above,
                                                              unsigned long long* __restrict__ nan_count,
                                                              unsigned long long* __restrict__ status_counts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_total) return;
  const int64_t p = i / frames_per_point;
  const int b = hest_bin(frame_nmse[i], thr, n_bins);
  atomicAdd(b >= 0 ? hist + p * n_bins + b : b == HEST_BIN_BELOW ? below + p : b == HEST_BIN_ABOVE ? above + p : nan_count + p, 1ull);
  const int st = status[i];
  atomicAdd(status_counts + 4 * p + (st == 0 ? 0 : st == 1 ? 1 : st == -1 ? 2 : 3), 1ull);
}

// the chunk's rows from the arena's estimate; amp / amp_stride / dl: the frames' taps, or htab: the static channel's table
static int hest_capture_frames(const ofdm_rx_plan* pl, const HestPass& p, const T4Estimate& e, const c64* amp, int64_t amp_stride,
                               const TxfDelays& dl, const c64* htab, int64_t nf, const HestRows& o) {
  if (p.lanes * p.frames_per_wg != HEST_THREADS || p.frames_per_wg > HEST_MAX_FRAMES_PER_WG || p.lds != HEST_CAPTURE_LDS) {
    set_error("hest_capture_kernel: launch shape differs from the kernel's");
    return OFDM_ERR_STATE;
  }
  hipStream_t s = ctx().stream;
  const int32_t* pc0 = (const int32_t*)pl->d_pc0;
  if (pl->f64)
    hipLaunchKernelGGL(hest_capture_kernel<double>, dim3(p.grid), dim3(p.threads), 0, s, (const c64*)e.H, (const c64*)e.hp, pc0, amp,
                       amp_stride, dl, htab, pl->nfft, pl->n_carrier, pl->np, p.lanes, nf, o);
  else
    hipLaunchKernelGGL(hest_capture_kernel<float>, dim3(p.grid), dim3(p.threads), 0, s, (const c32*)e.H, (const c32*)e.hp, pc0, amp,
                       amp_stride, dl, htab, pl->nfft, pl->n_carrier, pl->np, p.lanes, nf, o);
  return check_launch("hest_capture_kernel");
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_hest(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int time_desync, int freq_desync, void* h_est_out,
                            void* h_pilots_out, int64_t* tg_position_out, double* freq_offset_out, int32_t* ifo_out,
                            int32_t* status_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  HestCapture cap;
  cap.time_desync = time_desync;
  cap.freq_desync = freq_desync;
  cap.out = h_est_out || h_pilots_out || tg_position_out || freq_offset_out || ifo_out || status_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(hest_rx_prelude(pl ? &s : nullptr, rx != nullptr, is_f64(flags), n_frames, cap, why), why));
  if (n_frames == 0) return OFDM_OK;
  const size_t nf = (size_t)n_frames, cs = csize(flags), nc = (size_t)pl->n_carrier, np = (size_t)pl->np;
  const size_t frame_samples = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  const void* drx;
  void *dh, *dhp, *dtg, *dfo, *difo, *dst;
  OFDM_TRY(st.in(rx, cs * frame_samples * nf, &drx));
  OFDM_TRY(st.out(h_est_out, cs * nc * nf, &dh));
  OFDM_TRY(st.out(h_pilots_out, cs * np * nf, &dhp));
  // the scalars are always produced (scratch when the caller does not want them)
  auto scalar = [&st](void* user, size_t bytes, void** d) { return user ? st.out(user, bytes, d) : st.scratch(bytes, d); };
  OFDM_TRY(scalar(tg_position_out, sizeof(int64_t) * nf, &dtg));
  OFDM_TRY(scalar(freq_offset_out, sizeof(double) * nf, &dfo));
  OFDM_TRY(scalar(ifo_out, sizeof(int32_t) * nf, &difo));
  OFDM_TRY(scalar(status_out, sizeof(int32_t) * nf, &dst));
  for (int64_t f0 = 0; f0 < n_frames; f0 += 65535) {                       // a receiver call holds at most 65535 frames
    const int64_t n = std::min<int64_t>(65535, n_frames - f0);
    T4Estimate e{};
    OFDM_TRY(task4_estimate(pl, (const unsigned char*)drx + cs * frame_samples * (size_t)f0, n, time_desync, freq_desync,
                            (int64_t*)dtg + f0, (double*)dfo + f0, (int32_t*)difo + f0, (int32_t*)dst + f0, &e));
    // the arena's rows as they are: what h_out of the receiver copies, and the rows the spline operator read
    if (dh) OFDM_HIP(hipMemcpyAsync((unsigned char*)dh + cs * nc * (size_t)f0, e.H, cs * nc * (size_t)n, hipMemcpyDeviceToDevice, stream));
    if (dhp) OFDM_HIP(hipMemcpyAsync((unsigned char*)dhp + cs * np * (size_t)f0, e.hp, cs * np * (size_t)n, hipMemcpyDeviceToDevice, stream));
  }
  return st.finish();
}

extern "C" int ofdm_hest_study(ofdm_rx_plan* pl, const void* h, int h_len, const int32_t* tap_delay, const double* tap_power,
                               int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                               int freq_desync, const uint8_t* scr_reg15, const double* snr_db, const uint64_t* seeds,
                               int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                               int hist_bins, double hist_lo_db, double hist_hi_db, double* est_amp_sums_out,
                               double* true_amp_sums_out, double* err_sums_out, double* amp_err_sums_out, uint64_t* dropped_out,
                               double* pilot_amp_sums_out, double* pilot_err_sums_out, uint64_t* pilot_dropped_out,
                               double* nmse_sums_out, double* amp_nmse_sums_out, double* frame_nmse_out, double* frame_amp_nmse_out,
                               uint64_t* nmse_hist_out, uint64_t* nmse_below_out, uint64_t* nmse_above_out, uint64_t* nmse_nan_out,
                               uint64_t* status_counts_out, double* thresholds_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs a{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  const bool fading = a.fading();
  HestCapture cap;
  cap.time_desync = time_desync;
  cap.freq_desync = freq_desync;
  cap.study = true;
  cap.bins.n = hist_bins; cap.bins.lo = hist_lo_db; cap.bins.hi = hist_hi_db;
  cap.out = est_amp_sums_out || true_amp_sums_out || err_sums_out || amp_err_sums_out || dropped_out || pilot_amp_sums_out ||
            pilot_err_sums_out || pilot_dropped_out || nmse_sums_out || amp_nmse_sums_out || frame_nmse_out || frame_amp_nmse_out ||
            nmse_hist_out || nmse_below_out || nmse_above_out || nmse_nan_out || status_counts_out || thresholds_out;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(hest_study_prelude(a.call("hest_study", pl ? &s : nullptr), a.both_channels(), cap, ch, fade.gains, why), why));
  const size_t nc = (size_t)pl->n_carrier, npil = (size_t)pl->np, np = (size_t)n_points, fpp = (size_t)frames_per_point;
  const size_t nb = (size_t)hist_bins, NF = np * fpp;
  // the table of linear thresholds: made once, on the host; host memory whatever the flags
  std::vector<double> thr(nb + 1);
  hest_thresholds(cap.bins, pl->n_carrier, thr.data());
  if (thresholds_out) std::copy(thr.begin(), thr.end(), thresholds_out);
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  void *dfn, *dfa;
  OFDM_TRY(st.out(frame_nmse_out, sizeof(double) * NF, &dfn));
  OFDM_TRY(st.out(frame_amp_nmse_out, sizeof(double) * NF, &dfa));
  if (n_points == 0) return st.finish();
  double *dsum[4], *dpsum[2], *dns, *dans;
  unsigned long long *ddrop, *dpdrop, *dhist, *dbelow, *dabove, *dnan, *dstc;
  OFDM_TRY(txf_table(st, est_amp_sums_out, nc * np, dsum[0]));
  OFDM_TRY(txf_table(st, true_amp_sums_out, nc * np, dsum[1]));
  OFDM_TRY(txf_table(st, err_sums_out, nc * np, dsum[2]));
  OFDM_TRY(txf_table(st, amp_err_sums_out, nc * np, dsum[3]));
  OFDM_TRY(txf_table(st, dropped_out, nc * np, ddrop));
  OFDM_TRY(txf_table(st, pilot_amp_sums_out, npil * np, dpsum[0]));
  OFDM_TRY(txf_table(st, pilot_err_sums_out, npil * np, dpsum[1]));
  OFDM_TRY(txf_table(st, pilot_dropped_out, npil * np, dpdrop));
  OFDM_TRY(txf_table(st, nmse_sums_out, np, dns));
  OFDM_TRY(txf_table(st, amp_nmse_sums_out, np, dans));
  OFDM_TRY(txf_table(st, nmse_hist_out, nb * np, dhist));
  OFDM_TRY(txf_table(st, nmse_below_out, np, dbelow));
  OFDM_TRY(txf_table(st, nmse_above_out, np, dabove));
  OFDM_TRY(txf_table(st, nmse_nan_out, np, dnan));
  OFDM_TRY(txf_table(st, status_counts_out, 4 * np, dstc));
  if (frames_per_point == 0) return st.finish();
  if (!dfn) OFDM_TRY(st.scratch(sizeof(double) * NF, &dfn));
  if (!dfa) OFDM_TRY(st.scratch(sizeof(double) * NF, &dfa));
  const int taps = (int)ch.delay.size();
  const TxfUse u = a.use(ch);
  const int64_t CH = hest_chunk(s, u, frames_per_point, max_frames_per_chunk);
  const size_t chn = (size_t)CH;
  void *car, *cmask, *pil, *pmask, *ctg, *cfo, *cifo, *dstat, *dthr, *dstatic = nullptr, *dtab = nullptr;
  OFDM_TRY(st.scratch(sizeof(double) * HEST_CARRIER_ROWS * nc * chn, &car));
  OFDM_TRY(st.scratch(nc * chn, &cmask));
  OFDM_TRY(st.scratch(sizeof(double) * HEST_PILOT_ROWS * npil * chn, &pil));
  OFDM_TRY(st.scratch(npil * chn, &pmask));
  OFDM_TRY(st.scratch(sizeof(int64_t) * chn, &ctg));
  OFDM_TRY(st.scratch(sizeof(double) * chn, &cfo));
  OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &cifo));
  OFDM_TRY(st.scratch(sizeof(int32_t) * NF, &dstat));                    // every frame's status, counted after the last chunk
  OFDM_TRY(st.scratch(sizeof(double) * (nb + 1), &dthr));
  OFDM_TRY(study_thresholds_device(thr.data(), nb + 1, (double*)dthr));
  const TxfDelays dl = txf_delays(ch);
  if (!fading) {                                                          // a static channel: its taps and its H(k), once
    OFDM_TRY(st.scratch(sizeof(c64) * (size_t)std::max(taps, 1), &dstatic));   // an all-zero h has no taps: H = 0
    OFDM_TRY(txf_static_amps(ch, (c64*)dstatic));
    OFDM_TRY(st.scratch(sizeof(c64) * nc, &dtab));
    hipLaunchKernelGGL(hest_static_table_kernel, dim3(cdiv_u(pl->n_carrier, 256)), dim3(256), 0, stream, (const c64*)dstatic, dl,
                       pl->nfft, pl->n_carrier, (c64*)dtab);
    OFDM_TRY(check_launch("hest_static_table_kernel"));
  }
  const HestPass hp = hest_pass(s, CH);
  const HestRows rows{(double*)car, (uint8_t*)cmask, (double*)pil, (uint8_t*)pmask};
  const TxfImp imp = a.imp();
  OFDM_TRY(txf_sweep_points(pl, ch, a.points(), scr_reg15, CH, a.imp_on() ? &imp : nullptr, fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    HestSums cs{}, ps{};
    for (int q = 0; q < 4; ++q) cs.sums[q] = dsum[q] + nc * (size_t)p;
    cs.dropped = ddrop + nc * (size_t)p;
    for (int q = 0; q < 2; ++q) ps.sums[q] = dpsum[q] + npil * (size_t)p;
    ps.dropped = dpdrop + npil * (size_t)p;
    T4Estimate e{};
    OFDM_TRY(task4_estimate(pl, b.rx, nf, time_desync, freq_desync, (int64_t*)ctg, (double*)cfo, (int32_t*)cifo,
                            (int32_t*)dstat + at, &e));
    const c64* const amp = fading ? (const c64*)b.amp : (const c64*)dstatic;
    const int64_t stride = fading ? taps : 0;
    // the sweeps' own error sum on the estimate the equaliser would read
    OFDM_TRY(txf_frame_nmse(pl, amp, e.H, dl, stride, nf, (double*)dfn + at));
    OFDM_TRY(hest_capture_frames(pl, hp, e, amp, stride, dl, (const c64*)dtab, nf, rows));
    hipLaunchKernelGGL(hest_frame_sum_kernel, dim3((unsigned)nf), dim3(256), 0, stream, (const double*)car, pl->n_carrier,
                       (double*)dfa + at);
    hipLaunchKernelGGL(hest_accumulate_kernel, dim3(hp.acc_grid, (unsigned)HEST_CARRIER_ROWS), dim3(hp.acc_threads), 0, stream,
                       (const double*)car, (const uint8_t*)cmask, nf, (int)HEST_CARRIER_ROWS, pl->n_carrier, cs);
    hipLaunchKernelGGL(hest_accumulate_kernel, dim3(hp.acc_grid_pilots, (unsigned)HEST_PILOT_ROWS), dim3(hp.acc_threads), 0, stream,
                       (const double*)pil, (const uint8_t*)pmask, nf, (int)HEST_PILOT_ROWS, pl->np, ps);
    return check_launch("hest_accumulate_kernel");
  }));
  OFDM_TRY(txf_point_sums1(dfn, n_points, frames_per_point, dns));
  OFDM_TRY(txf_point_sums1(dfa, n_points, frames_per_point, dans));
  hipLaunchKernelGGL(hest_frame_hist_kernel, dim3(cdiv_u((int64_t)NF, 256)), dim3(256), 0, stream, (const double*)dfn,
                     (const int32_t*)dstat, frames_per_point, (int64_t)NF, (const double*)dthr, hist_bins, dhist, dbelow, dabove, dnan,
                     dstc);
  OFDM_TRY(check_launch("hest_frame_hist_kernel"));
  return st.finish();
}
