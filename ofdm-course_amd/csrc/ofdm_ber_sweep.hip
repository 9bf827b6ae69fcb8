// ofdm_ber_sweep_task5 / ofdm_ber_sweep_task4: one device-resident tile of a BER(SNR) sweep on top of the fused frame generator
// of ofdm_txfused.hip (T3/Main_model_Task_3.m:237-268, T5/Task5_part2.m:134,:148-152): per point and chunk the frames are
// generated into the plan-owned workspace (txf_generate) and decoded in place by the Task-5 or the Task-4 receiver.
//
//   ber_point_reduce_kernel         per-frame uint32 errors -> per-point uint64 (integers: exact in any order).
//   t4_point_reduce_kernel          per-frame errors / status / |FreqOffset + IFO - Freq_Shift| of a whole point -> its sums,
//                                   in a fixed order (the double sum does not depend on the chunking).
//   t4_point_mer_kernel             per-frame MER_func sums -> per-point sums in the same fixed order (both sweeps with MER).
//   t5_frame_nmse_kernel<T>         one workgroup per frame: H_f(k) = sum_t a_t e^{-2 pi i d_t k / Nfft} in double (the phase
//                                   d_t k mod Nfft reduced in integers), sum_k |H_f(k) - Hest_f(k)|^2 over 1..N_carrier in a
//                                   fixed order (T5/Task5_part2.m:202-205); the points through t4_point_mer_kernel<1>
//   tx_static_amp_kernel            the static channel's taps into device memory once per sweep, so that t5_frame_nmse_kernel
//                                   reads them with a frame stride of 0 (ofdm_ber_sweep_task4_nmse, NMSE of T4:205-239)
//
// Host side: what a call decides -- its channel, the chunk, the argument checks in the entry's order -- is txf_plan.hpp's.
// The two sweep bodies (t5_sweep, t4_sweep) share the staging of the outputs both have -- errors, MER sums, channel-estimate
// error sums, per point and per frame (SweepOuts, txf_sweep_outputs) --, the point x chunk loop with the generation inside
// (txf_sweep_points of txf_study.hpp, the receiver passed as a callable), the fixed-order sums of the per-frame doubles
// (txf_point_sums) and the constellation density (SweepScope; SweepScopeAcc owns where the grids live, their zeroing, the
// capture of a receiver call and the copy back).  Each keeps its receiver's own outputs, scratch, chunk budget and per-point
// reduction.  Every extern "C" entry is one call of its receiver's t5_entry / t4_entry, which fills the TxfCall from the
// entry's channel (SweepChan: a static h, or a tap-delay line, for which the generator draws a channel per frame), points and
// outputs, or forwards to the entry whose arguments contain its own.
#include <algorithm>
#include <cmath>

#include "channel_resp.hpp"
#include "scope_plan.hpp"
#include "txf_study.hpp"

namespace ofdm {

int scope_refused(int id, const ScopeWhy& w);                     // ofdm_chain_t4.hip

// the taps of a static channel (host doubles in the kernel arguments) -> device memory, for t5_frame_nmse_kernel
struct TxfAmps {
  c64 a[TXF_MAX_TAPS];
};

__global__ __launch_bounds__(64) void tx_static_amp_kernel(c64* __restrict__ amp, TxfAmps amps, int n_taps) {
  if ((int)threadIdx.x < n_taps) amp[threadIdx.x] = amps.a[threadIdx.x];
}

// per frame f of a fading sweep: sum_{k < n_carrier} |H_f(k) - hest[f][k]|^2 with H_f(k) = sum_t a_{f,t} e^{-2 pi i d_t k / Nfft}
// = fft(h_f, Nfft)(k) of get_MP_channel_resp (T5/Task5_part2.m:160-166,:202-205), in double.  One workgroup per frame: each
// thread a fixed stride of carriers, a fixed butterfly, the four wave partials paired -- no atomics.
// amp_stride: dl.n for the amplitudes of a channel per frame [frames][dl.n], 0 for one static channel [dl.n].  H_f(k):
// channel_resp (channel_resp.hpp), shared with the channel study.

template <typename T>
__global__ __launch_bounds__(256) void t5_frame_nmse_kernel(const c64* __restrict__ amp, const cx<T>* __restrict__ hest,
                                                            TxfDelays dl, int64_t amp_stride, int nfft, int n_carrier,
                                                            double* __restrict__ frame_nmse) {
  __shared__ c64 a[TXF_MAX_TAPS];
  __shared__ double part[4];
  const int64_t f = blockIdx.x;
  if ((int)threadIdx.x < dl.n) a[threadIdx.x] = amp[f * amp_stride + threadIdx.x];
  __syncthreads();
  const double inv = 2.0 / (double)nfft;
  double s = 0;
  for (int k = threadIdx.x; k < n_carrier; k += 256) {
    double hr, hi;
    channel_resp(a, dl, k, nfft, inv, hr, hi);
    const cx<T> e = hest[f * n_carrier + k];
    const double dr = hr - (double)e.x, di = hi - (double)e.y;
    s += dr * dr + di * di;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) frame_nmse[f] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(256) void ber_point_reduce_kernel(const uint32_t* __restrict__ frame_errors,
                                                               int64_t frames_per_point,
                                                               unsigned long long* __restrict__ errors) {
  const int64_t p = blockIdx.x;
  unsigned long long s = 0;
  for (int64_t i = threadIdx.x; i < frames_per_point; i += 256) s += frame_errors[p * frames_per_point + i];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  __shared__ unsigned long long part[4];
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) errors[p] = part[0] + part[1] + part[2] + part[3];
}

// per point p of a Task-4 sweep: bit errors (uint64), status counts {0, 1, -1, -2} and, with freq_desync, the sum of
// |FreqOffset + IFO - Freq_Shift| (T4/Main_model_Task_4.m:113-134) over the point's frames -- each thread a fixed stride,
// then a fixed butterfly: the same order for any chunking of the frames
__global__ __launch_bounds__(256) void t4_point_reduce_kernel(const uint32_t* __restrict__ frame_errors,
                                                              const int32_t* __restrict__ status, const double* __restrict__ fo,
                                                              const int32_t* __restrict__ ifo, const double* __restrict__ shift,
                                                              int64_t frames_per_point, int freq_desync,
                                                              unsigned long long* __restrict__ errors,
                                                              unsigned long long* __restrict__ status_counts,
                                                              double* __restrict__ cfo_abs_err) {
  const int64_t p = blockIdx.x;
  unsigned long long e = 0, c[4] = {0, 0, 0, 0};
  double a = 0;
  for (int64_t i = threadIdx.x; i < frames_per_point; i += 256) {
    const int64_t k = p * frames_per_point + i;
    e += frame_errors[k];
    const int st = status[k];
    c[st == 0 ? 0 : st == 1 ? 1 : st == -1 ? 2 : 3] += 1;
    if (freq_desync) a += fabs(fo[k] + (double)ifo[k] - shift[k]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    e += __shfl_xor(e, off, 64);
    for (int q = 0; q < 4; ++q) c[q] += __shfl_xor(c[q], off, 64);
    a += __shfl_xor(a, off, 64);
  }
  __shared__ unsigned long long pe[4], pc[4][4];
  __shared__ double pa[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    pe[w] = e;
    for (int q = 0; q < 4; ++q) pc[w][q] = c[q];
    pa[w] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    errors[p] = pe[0] + pe[1] + pe[2] + pe[3];
    if (status_counts)
      for (int q = 0; q < 4; ++q) status_counts[p * 4 + q] = pc[0][q] + pc[1][q] + pc[2][q] + pc[3][q];
    if (cfo_abs_err) cfo_abs_err[p] = (pa[0] + pa[1]) + (pa[2] + pa[3]);
  }
}

// per point p of a Task-4 / Task-5 sweep with MER: the per-frame MER_func sums {s1, s2} of the symbol stages' MER variants -> the
// point's {sum s1, sum s2} (MER_func of the point's RX_IQ concatenated) -- the fixed order of t4_point_reduce_kernel:
// each thread a fixed stride, a fixed butterfly, the four wave partials paired; bitwise independent of the chunking.
// W = values per frame: 2 for the MER sums, 1 for the channel-estimate error of a fading sweep (t5_frame_nmse_kernel).
template <int W>
__global__ __launch_bounds__(256) void t4_point_mer_kernel(const double* __restrict__ frame_mer, int64_t frames_per_point,
                                                           double* __restrict__ mer_sums) {
  const int64_t p = blockIdx.x;
  double a[W];
  for (int q = 0; q < W; ++q) a[q] = 0;
  for (int64_t i = threadIdx.x; i < frames_per_point; i += 256) {
    const int64_t k = p * frames_per_point + i;
    for (int q = 0; q < W; ++q) a[q] += frame_mer[W * k + q];
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int q = 0; q < W; ++q) a[q] += __shfl_xor(a[q], off, 64);
  __shared__ double pa[4][W];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < W; ++q) pa[w][q] = a[q];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int q = 0; q < W; ++q) mer_sums[W * p + q] = (pa[0][q] + pa[1][q]) + (pa[2][q] + pa[3][q]);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

// what a caller of a sweep may ask for beside its receiver's own outputs: per point the bit errors, the MER sums and the
// channel-estimate error sums, per frame the same three (errors: mandatory; every other: null = not wanted)
struct SweepOuts {
  uint64_t* errors;
  uint32_t* frame_errors;
  double *mer_sums, *frame_mer_sums, *nmse_sums, *frame_nmse;
};

// those outputs as the kernels see them
struct TxfSweepOut {
  void *err = nullptr, *fe = nullptr, *mer = nullptr, *fm = nullptr, *ns = nullptr, *fn = nullptr;
};

// stages the common outputs; with no frames the per-point sums are zeroed, else the per-frame values of every point
// (reduced once after the last chunk) get scratch where the caller wants none
static int txf_sweep_outputs(Stage& st, int64_t n_points, int64_t frames_per_point, const SweepOuts& out, TxfSweepOut& o) {
  const size_t np = (size_t)n_points, nf = (size_t)(n_points * frames_per_point);
  OFDM_TRY(st.out(out.errors, sizeof(uint64_t) * np, &o.err));
  OFDM_TRY(st.out(out.frame_errors, sizeof(uint32_t) * nf, &o.fe));
  OFDM_TRY(st.out(out.mer_sums, sizeof(double) * 2 * np, &o.mer));
  OFDM_TRY(st.out(out.frame_mer_sums, sizeof(double) * 2 * nf, &o.fm));
  OFDM_TRY(st.out(out.nmse_sums, sizeof(double) * np, &o.ns));
  OFDM_TRY(st.out(out.frame_nmse, sizeof(double) * nf, &o.fn));
  if (frames_per_point == 0) {
    OFDM_HIP(hipMemsetAsync(o.err, 0, sizeof(uint64_t) * np, ctx().stream));
    if (o.mer) OFDM_HIP(hipMemsetAsync(o.mer, 0, sizeof(double) * 2 * np, ctx().stream));
    if (o.ns) OFDM_HIP(hipMemsetAsync(o.ns, 0, sizeof(double) * np, ctx().stream));
    return OFDM_OK;
  }
  if (!o.fe) OFDM_TRY(st.scratch(sizeof(uint32_t) * nf, &o.fe));
  if (o.mer && !o.fm) OFDM_TRY(st.scratch(sizeof(double) * 2 * nf, &o.fm));
  if (o.ns && !o.fn) OFDM_TRY(st.scratch(sizeof(double) * nf, &o.fn));
  return OFDM_OK;
}

// the per-point sums of W doubles per frame, in a fixed order: the MER sums (W = 2), the channel-estimate errors (W = 1)
template <int W>
static int txf_point_sums(const void* frame_values, int64_t n_points, int64_t frames_per_point, void* sums) {
  if (!sums) return OFDM_OK;
  hipLaunchKernelGGL(t4_point_mer_kernel<W>, dim3((unsigned)n_points), dim3(256), 0, ctx().stream, (const double*)frame_values,
                     frames_per_point, (double*)sums);
  return check_launch("t4_point_mer_kernel");
}

// the W = 1 sum for callers outside this file (the channel study: its two per-frame error sums)
int txf_point_sums1(const void* frame_values, int64_t n_points, int64_t frames_per_point, void* sums) {
  return txf_point_sums<1>(frame_values, n_points, frames_per_point, sums);
}

// the taps of a static channel into damp (room for max(taps, 1) amplitudes): what txf_frame_nmse reads with a frame stride of 0
int txf_static_amps(const TxfChannel& ch, c64* damp) {
  const int n_taps = (int)ch.delay.size();
  TxfAmps sa{};
  for (int t = 0; t < n_taps; ++t) sa.a[t] = mk<double>(ch.amp[t].x, ch.amp[t].y);
  hipLaunchKernelGGL(tx_static_amp_kernel, dim3(1), dim3(64), 0, ctx().stream, damp, sa, n_taps);
  return check_launch("tx_static_amp_kernel");
}

// the channel-estimate error of the chunk's nf frames against the channel of taps dl / amplitudes amp (t5_frame_nmse_kernel)
int txf_frame_nmse(const ofdm_rx_plan* pl, const c64* amp, const void* hest, const TxfDelays& dl, int64_t amp_stride,
                          int64_t nf, double* frame_nmse) {
  if (pl->f64)
    hipLaunchKernelGGL(t5_frame_nmse_kernel<double>, dim3((unsigned)nf), dim3(256), 0, ctx().stream, amp, (const c64*)hest, dl,
                       amp_stride, pl->nfft, pl->n_carrier, frame_nmse);
  else
    hipLaunchKernelGGL(t5_frame_nmse_kernel<float>, dim3((unsigned)nf), dim3(256), 0, ctx().stream, amp, (const c32*)hest, dl,
                       amp_stride, pl->nfft, pl->n_carrier, frame_nmse);
  return check_launch("t5_frame_nmse_kernel");
}

TxfDelays txf_delays(const TxfChannel& ch) {
  TxfDelays dl{};
  dl.n = (int)ch.delay.size();
  for (int t = 0; t < dl.n; ++t) dl.d[t] = ch.delay[t];
  return dl;
}

// the checked prelude of a sweep entry: c completed from the plan, the flags and the mandatory output, then its checks
template <typename Prelude>
static int txf_sweep_prelude(ofdm_rx_plan* pl, TxfCall& c, TxfShape& s, const void* errors_out, int flags, Prelude prelude,
                             TxfChannel& ch, TxfFade& fade) {
  OFDM_TRY(ensure_init());
  if (pl) s = txf_shape(pl);
  c.plan = pl ? &s : nullptr;
  c.out = errors_out != nullptr;
  c.f64_flag = is_f64(flags);
  TxfWhy why;
  return txf_refused(prelude(c, ch, fade.gains, why), why);
}

// the constellation density of a sweep's points (ofdm_ber_sweep_task5_scope, ofdm_ber_sweep_task4_scope)
struct SweepScope {
  bool on = false;
  int bins = 0;
  double half_width = 0.0;
  int64_t skip = 0;
  uint64_t *density_out = nullptr, *dropped_out = nullptr;
  SweepScope() = default;
  SweepScope(int bins_, double half_width_, int64_t skip_, uint64_t* density_out_, uint64_t* dropped_out_)
      : on(true), bins(bins_), half_width(half_width_), skip(skip_), density_out(density_out_), dropped_out(dropped_out_) {}
};

// The density grids [n_points][bins][bins] and the dropped counters [n_points] are accumulators of the global atomics of the
// Task-5 symbol stages and of the Task-4 receiver's eq_demap_kernel: the caller's device outputs themselves; host outputs, and
// dropped counters nobody asked for, in a buffer of the plan's own (pl->ws_scope -- not the generator workspace, whose regions
// are per chunk).  Zeroed on the launch stream before the first chunk; host outputs are copied back in front of st.finish()'s
// synchronisation (finish()).
struct SweepScopeAcc {
  unsigned long long *dens = nullptr, *drop = nullptr;
  size_t grid_elems = 0;
  int begin(ofdm_rx_plan* pl, const SweepScope& a, bool device_mode, int64_t n_points) {
    hipStream_t stream = ctx().stream;
    grid_elems = (size_t)a.bins * (size_t)a.bins;
    const size_t own = sizeof(uint64_t) * (device_mode ? (a.dropped_out ? 0 : (size_t)n_points) : (size_t)n_points * (grid_elems + 1));
    if (pl->ws_scope_bytes < own) {
      OFDM_HIP(hipStreamSynchronize(stream));
      if (pl->ws_scope) { (void)hipFree(pl->ws_scope); pl->ws_scope = nullptr; pl->ws_scope_bytes = 0; }
      OFDM_HIP(hipMalloc(&pl->ws_scope, own));
      pl->ws_scope_bytes = own;
    }
    if (device_mode) {
      dens = (unsigned long long*)a.density_out;
      drop = a.dropped_out ? (unsigned long long*)a.dropped_out : (unsigned long long*)pl->ws_scope;
    } else {
      dens = (unsigned long long*)pl->ws_scope;
      drop = dens + (size_t)n_points * grid_elems;
    }
    OFDM_HIP(hipMemsetAsync(dens, 0, sizeof(uint64_t) * (size_t)n_points * grid_elems, stream));
    OFDM_HIP(hipMemsetAsync(drop, 0, sizeof(uint64_t) * (size_t)n_points, stream));
    return OFDM_OK;
  }
  // the capture of a receiver call on frames of point p (a chunk holds frames of one point: one grid per call)
  ScopeCall call(const SweepScope& a, int64_t p) const {
    ScopeCall sc;
    sc.bins = a.bins; sc.skip = a.skip; sc.half_width = a.half_width;
    sc.scale = scope_scale(a.bins, a.half_width);
    sc.density = dens + (size_t)p * grid_elems; sc.dropped = drop + p;
    return sc;
  }
  int finish(const SweepScope& a, bool device_mode, int64_t n_points) const {
    if (device_mode) return OFDM_OK;
    hipStream_t stream = ctx().stream;
    OFDM_HIP(hipMemcpyAsync(a.density_out, dens, sizeof(uint64_t) * (size_t)n_points * grid_elems, hipMemcpyDeviceToHost, stream));
    if (a.dropped_out) OFDM_HIP(hipMemcpyAsync(a.dropped_out, drop, sizeof(uint64_t) * (size_t)n_points, hipMemcpyDeviceToHost, stream));
    return OFDM_OK;
  }
};

// the body of the Task-5 sweep entries: the checks of txf_task5_prelude, then c's static channel, or the delay line of a
// channel per frame; out.nmse_sums / out.frame_nmse (fading only): the channel-estimate error sums; sw: the density of
// ofdm_ber_sweep_task5_scope
static int t5_sweep(ofdm_rx_plan* pl, TxfCall c, const SweepOuts& out, int flags, const SweepScope& sw) {
  TxfShape s{};
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_sweep_prelude(pl, c, s, out.errors, flags, txf_task5_prelude, ch, fade));
  const int64_t decisions = (int64_t)s.nd * s.n_symb;
  if (sw.on) {                                                  // behind every check of the entry without a density
    int stage = SYM_EQ_DEMAP;
    size_t stage_lds = 0;
    // (a plan the receiver refuses has no stage: the first receiver call says so in the receiver's words)
    const bool routed = rx_chain_task5_scope_stage(pl, &stage, &stage_lds);
    ScopeWhy why;
    OFDM_TRY(scope_refused(scope5_density_check(stage, routed ? stage_lds : 0, sw.bins, sw.half_width, sw.skip, decisions,
                                                sw.density_out != nullptr, why), why));
  }
  const TxfPoints pt{c.snr_db, c.seeds, c.n_points, c.n_frames, c.frame0};
  const int64_t n_points = pt.n_points, frames_per_point = pt.frames_per_point;
  if (n_points == 0) return OFDM_OK;
  Stage st(flags);
  TxfSweepOut o;
  OFDM_TRY(txf_sweep_outputs(st, n_points, frames_per_point, out, o));
  SweepScopeAcc acc;
  if (sw.on) OFDM_TRY(acc.begin(pl, sw, st.device_mode(), n_points));
  if (frames_per_point == 0) {
    if (sw.on) OFDM_TRY(acc.finish(sw, st.device_mode(), n_points));
    return st.finish();
  }
  TxfUse u;
  u.scr = c.scr_reg15 != nullptr;
  u.sweep = true;
  u.fade_taps = c.fading ? (int)ch.delay.size() : 0;
  u.hest = o.fn != nullptr;
  int64_t CH = txf_chunk(s, u, frames_per_point, c.max_chunk);
  // a density: a chunk holds at most 2^32 - 1 points, so that no uint32 bin of a workgroup's grid can wrap (counts are integers:
  // the result does not depend on the chunking)
  if (sw.on) CH = std::max<int64_t>(1, std::min<int64_t>(CH, (int64_t)(0xffffffffull / (unsigned long long)decisions)));
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  TxfDelays dl{};
  if (c.fading) dl = txf_delays(ch);
  // a plan in the h = ifft(H_LS) MMSE mode estimates every point at the point's own SNR (a host scalar of the stage's launch)
  OFDM_TRY(txf_sweep_points(pl, ch, pt, c.scr_reg15, CH, nullptr, c.fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t k) {
                              const double inv_snr = 1.0 / std::pow(10.0, pt.snr_db[p] * 0.1);
                              ScopeCall sc;
                              if (sw.on) sc = acc.call(sw, p);
                              OFDM_TRY(rx_chain_task5_run(pl, b.rx, nf, nullptr, (const uint8_t*)b.ref,
                                                          (uint32_t*)o.fe + k, b.hest, nullptr,
                                                          o.fm ? (double*)o.fm + 2 * k : nullptr, rxflags, inv_snr,
                                                          sw.on ? &sc : nullptr));
                              if (!o.fn) return (int)OFDM_OK;
                              return txf_frame_nmse(pl, b.amp, b.hest, dl, (int64_t)dl.n, nf, (double*)o.fn + k);
                            }));
  hipLaunchKernelGGL(ber_point_reduce_kernel, dim3((unsigned)n_points), dim3(256), 0, ctx().stream, (const uint32_t*)o.fe,
                     frames_per_point, (unsigned long long*)o.err);
  OFDM_TRY(check_launch("ber_point_reduce_kernel"));
  OFDM_TRY(txf_point_sums<2>(o.fm, n_points, frames_per_point, o.mer));
  OFDM_TRY(txf_point_sums<1>(o.fn, n_points, frames_per_point, o.ns));
  if (sw.on) OFDM_TRY(acc.finish(sw, st.device_mode(), n_points));
  return st.finish();
}

// what the Task-4 sweep entries pass on to the receiver and get back beside the common outputs
struct T4SweepArgs {
  TxfImp imp;
  int time_desync, freq_desync, mp_desync;
  uint64_t* status_counts_out;
  double* cfo_abs_err_out;
  SweepScope sw;                                                // ofdm_ber_sweep_task4_scope: the density of every point
};

// the body of the Task-4 sweep entries: the checks of txf_task4_prelude, then c's static channel, or the delay line of a
// channel per frame; out.nmse_sums / out.frame_nmse (optional): the channel-estimate error sums against the channel's H
// (static: one H for every frame) or the frame's own H_f (fading)
static int t4_sweep(ofdm_rx_plan* pl, TxfCall c, const T4SweepArgs& a, const SweepOuts& out, int flags) {
  const SweepScope& sw = a.sw;
  c.nmse_out = out.nmse_sums || out.frame_nmse;
  c.mp_desync = a.mp_desync;
  TxfShape s{};
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_sweep_prelude(pl, c, s, out.errors, flags, txf_task4_prelude, ch, fade));
  if (sw.on) {                                                  // behind every check of the entry without a density
    ScopeWhy why;
    OFDM_TRY(scope_refused(scope_density_check(sw.density_out != nullptr, sw.bins, sw.half_width, sw.skip, s.f64 != 0,
                                               s.n_carrier, (int64_t)s.nd * s.n_symb, why), why));
  }
  const TxfPoints pt{c.snr_db, c.seeds, c.n_points, c.n_frames, c.frame0};
  const int64_t n_points = pt.n_points, frames_per_point = pt.frames_per_point;
  if (n_points == 0) return OFDM_OK;
  Stage st(flags);
  const int64_t NF = n_points * frames_per_point;
  TxfSweepOut o;
  OFDM_TRY(txf_sweep_outputs(st, n_points, frames_per_point, out, o));
  void *dsc, *dabs;
  OFDM_TRY(st.out(a.status_counts_out, sizeof(uint64_t) * 4 * (size_t)n_points, &dsc));
  OFDM_TRY(st.out(a.cfo_abs_err_out, sizeof(double) * (size_t)n_points, &dabs));
  hipStream_t stream = ctx().stream;
  SweepScopeAcc acc;
  if (sw.on) OFDM_TRY(acc.begin(pl, sw, st.device_mode(), n_points));
  if (frames_per_point == 0) {
    if (dsc) OFDM_HIP(hipMemsetAsync(dsc, 0, sizeof(uint64_t) * 4 * (size_t)n_points, stream));
    if (dabs) OFDM_HIP(hipMemsetAsync(dabs, 0, sizeof(double) * (size_t)n_points, stream));
    if (sw.on) OFDM_TRY(acc.finish(sw, st.device_mode(), n_points));
    return st.finish();
  }
  // the per-frame values of every point, reduced once after the last chunk
  void *dtg, *dfo, *difo, *dstat, *dsto, *dcfo;
  OFDM_TRY(st.scratch(sizeof(int64_t) * (size_t)NF, &dtg));
  OFDM_TRY(st.scratch(sizeof(double) * (size_t)NF, &dfo));
  OFDM_TRY(st.scratch(sizeof(int32_t) * (size_t)NF, &difo));
  OFDM_TRY(st.scratch(sizeof(int32_t) * (size_t)NF, &dstat));
  OFDM_TRY(st.scratch(sizeof(int64_t) * (size_t)NF, &dsto));
  OFDM_TRY(st.scratch(sizeof(double) * (size_t)NF, &dcfo));
  const int n_taps = (int)ch.delay.size();
  TxfUse u;
  u.scr = c.scr_reg15 != nullptr;
  u.sweep = true;
  u.imp = true;
  u.fade_taps = c.fading ? n_taps : 0;
  u.hest = o.fn != nullptr;
  const int64_t CH = txf_chunk_task4(s, u, frames_per_point, c.max_chunk, o.fm != nullptr);
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  TxfImp imp = a.imp;
  imp.sto = (int64_t*)dsto;
  imp.cfo = (double*)dcfo;
  TxfDelays dl{};
  void* dstatic = nullptr;                                      // NMSE against a static channel: its taps, read with stride 0
  if (o.fn) {
    dl = txf_delays(ch);
    if (!c.fading) {
      OFDM_TRY(st.scratch(sizeof(c64) * (size_t)std::max(n_taps, 1), &dstatic));   // an all-zero h has no taps: H = 0
      OFDM_TRY(txf_static_amps(ch, (c64*)dstatic));
    }
  }
  OFDM_TRY(txf_sweep_points(pl, ch, pt, c.scr_reg15, CH, &imp, c.fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t k) {
                              ScopeCall sc;
                              if (sw.on) sc = acc.call(sw, p);
                              OFDM_TRY(rx_chain_task4_run(pl, b.rx, nf, a.time_desync, a.freq_desync, a.mp_desync, nullptr,
                                                          (const uint8_t*)b.ref, (uint32_t*)o.fe + k, (int64_t*)dtg + k,
                                                          (double*)dfo + k, (int32_t*)difo + k, (int32_t*)dstat + k,
                                                          b.hest, c.mer_skip, o.fm ? (double*)o.fm + 2 * k : nullptr,
                                                          sw.on ? &sc : nullptr, rxflags));
                              if (!o.fn) return (int)OFDM_OK;
                              return txf_frame_nmse(pl, c.fading ? (const c64*)b.amp : (const c64*)dstatic, b.hest, dl,
                                                    c.fading ? n_taps : 0, nf, (double*)o.fn + k);
                            }));
  hipLaunchKernelGGL(t4_point_reduce_kernel, dim3((unsigned)n_points), dim3(256), 0, stream, (const uint32_t*)o.fe,
                     (const int32_t*)dstat, (const double*)dfo, (const int32_t*)difo, (const double*)dcfo, frames_per_point,
                     a.freq_desync ? 1 : 0, (unsigned long long*)o.err, (unsigned long long*)dsc, (double*)dabs);
  OFDM_TRY(check_launch("t4_point_reduce_kernel"));
  OFDM_TRY(txf_point_sums<2>(o.fm, n_points, frames_per_point, o.mer));
  OFDM_TRY(txf_point_sums<1>(o.fn, n_points, frames_per_point, o.ns));
  if (sw.on) OFDM_TRY(acc.finish(sw, st.device_mode(), n_points));
  return st.finish();
}

// what every sweep entry builds its TxfCall from: the channel as the static h / h_len or, with `fading`, as a tap-delay line
struct SweepChan {
  bool fading;
  const void* h;
  int h_len;
  const int32_t* tap_delay;
  const double* tap_power;
  int n_taps;
};
static SweepChan chan_static(const void* h, int h_len) { return SweepChan{false, h, h_len, nullptr, nullptr, 0}; }
static SweepChan chan_fading(const int32_t* tap_delay, const double* tap_power, int n_taps) {
  return SweepChan{true, nullptr, 0, tap_delay, tap_power, n_taps};
}

static TxfCall sweep_call(const char* what, const SweepChan& ch, const TxfPoints& pt, const uint8_t* scr_reg15, int64_t max_chunk) {
  TxfCall c(what, pt.frame0, pt.frames_per_point, scr_reg15);
  if (ch.fading) c.with_fading(ch.tap_delay, ch.tap_power, ch.n_taps);
  else c.with_h(ch.h, ch.h_len);
  return c.with_points(pt.snr_db, pt.seeds, pt.n_points, max_chunk);
}

// the one body of the Task-5 entries
static int t5_entry(ofdm_rx_plan* pl, const SweepChan& ch, const TxfPoints& pt, const uint8_t* scr_reg15, int64_t max_chunk,
                    const SweepOuts& out, int flags, const SweepScope& sw = SweepScope{}) {
  return t5_sweep(pl, sweep_call(ch.fading ? "ber_sweep_task5_fading" : "ber_sweep_task5", ch, pt, scr_reg15, max_chunk), out,
                  flags, sw);
}

// the one body of the Task-4 entries; a: the impairments, the receiver's flags and outputs, the density
static int t4_entry(ofdm_rx_plan* pl, const SweepChan& ch, const TxfPoints& pt, const uint8_t* scr_reg15, int64_t max_chunk,
                    int64_t mer_skip, const T4SweepArgs& a, const SweepOuts& out, int flags) {
  TxfCall c = sweep_call(ch.fading ? "ber_sweep_task4_fading" : "ber_sweep_task4", ch, pt, scr_reg15, max_chunk)
                  .with_imp(a.imp.sto_mode, a.imp.cfo_mode);
  c.mer_skip = mer_skip;
  return t4_sweep(pl, c, a, out, flags);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_ber_sweep_task5_ex(ofdm_rx_plan* pl, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                                       int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                       int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                                       double* mer_sums_out, double* frame_mer_sums_out, int flags) {
  return t5_entry(pl, chan_static(h, h_len), TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0}, scr_reg15,
                  max_frames_per_chunk, SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nullptr, nullptr},
                  flags);
}

extern "C" int ofdm_ber_sweep_task5_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                           const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                           int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                           int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                                           double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                           double* frame_nmse_out, int flags) {
  return t5_entry(pl, chan_fading(tap_delay, tap_power, n_taps), TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0},
                  scr_reg15, max_frames_per_chunk,
                  SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out}, flags);
}

extern "C" int ofdm_ber_sweep_task5_scope(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                          const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                          int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                          int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                                          double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                          double* frame_nmse_out, const void* h, int h_len, uint64_t* density_out,
                                          uint64_t* density_dropped_out, int bins, double half_width, int64_t scope_skip,
                                          int flags) {
  OFDM_TRY(ensure_init());
  // one channel: the static h / h_len (h = NULL: none), or the delay line of n_taps > 0 taps
  OFDM_ARG(!(n_taps > 0 && (h || h_len)), "ber_sweep_task5_scope: give the static channel h / h_len or the tap-delay line (n_taps > 0), not both");
  OFDM_ARG(n_taps >= 0, "ber_sweep_task5_scope: n_taps must be >= 0 (%d)", n_taps);
  OFDM_ARG(n_taps > 0 || (!nmse_sums_out && !frame_nmse_out), "ber_sweep_task5_scope: the NMSE outputs need the tap-delay line (n_taps > 0)");
  return t5_entry(pl, n_taps > 0 ? chan_fading(tap_delay, tap_power, n_taps) : chan_static(h, h_len),
                  TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0}, scr_reg15, max_frames_per_chunk,
                  SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out}, flags,
                  SweepScope(bins, half_width, scope_skip, density_out, density_dropped_out));
}

extern "C" int ofdm_ber_sweep_task5(ofdm_rx_plan* pl, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                                    int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                    int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out, int flags) {
  return ofdm_ber_sweep_task5_ex(pl, h, h_len, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15,
                                 max_frames_per_chunk, errors_out, frame_errors_out, nullptr, nullptr, flags);
}

extern "C" int ofdm_ber_sweep_task4_nmse(ofdm_rx_plan* pl, const void* h, int h_len, int sto_mode, int64_t sto_value,
                                         int cfo_mode, double cfo_value, int time_desync, int freq_desync, int mp_desync,
                                         const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                         int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                         int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* status_counts_out,
                                         double* cfo_abs_err_out, uint32_t* frame_errors_out, int64_t mer_skip,
                                         double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                         double* frame_nmse_out, int flags) {
  return t4_entry(pl, chan_static(h, h_len), TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0}, scr_reg15,
                  max_frames_per_chunk, mer_skip,
                  T4SweepArgs{TxfImp(sto_mode, sto_value, cfo_mode, cfo_value), time_desync, freq_desync, mp_desync,
                              status_counts_out, cfo_abs_err_out, SweepScope{}},
                  SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out}, flags);
}

extern "C" int ofdm_ber_sweep_task4_scope(ofdm_rx_plan* pl, const void* h, int h_len, int sto_mode, int64_t sto_value,
                                          int cfo_mode, double cfo_value, int time_desync, int freq_desync, int mp_desync,
                                          const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                          int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                          int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* status_counts_out,
                                          double* cfo_abs_err_out, uint32_t* frame_errors_out, int64_t mer_skip,
                                          double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                          double* frame_nmse_out, uint64_t* density_out, uint64_t* density_dropped_out, int bins,
                                          double half_width, int64_t scope_skip, int flags) {
  return t4_entry(pl, chan_static(h, h_len), TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0}, scr_reg15,
                  max_frames_per_chunk, mer_skip,
                  T4SweepArgs{TxfImp(sto_mode, sto_value, cfo_mode, cfo_value), time_desync, freq_desync, mp_desync,
                              status_counts_out, cfo_abs_err_out,
                              SweepScope(bins, half_width, scope_skip, density_out, density_dropped_out)},
                  SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out}, flags);
}

extern "C" int ofdm_ber_sweep_task4_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                           int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                                           int freq_desync, int mp_desync, const double* snr_db, const uint64_t* seeds,
                                           int64_t n_points, int64_t frames_per_point, int64_t frame0,
                                           const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                                           uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                                           int64_t mer_skip, double* mer_sums_out, double* frame_mer_sums_out,
                                           double* nmse_sums_out, double* frame_nmse_out, int flags) {
  return t4_entry(pl, chan_fading(tap_delay, tap_power, n_taps), TxfPoints{snr_db, seeds, n_points, frames_per_point, frame0},
                  scr_reg15, max_frames_per_chunk, mer_skip,
                  T4SweepArgs{TxfImp(sto_mode, sto_value, cfo_mode, cfo_value), time_desync, freq_desync, mp_desync,
                              status_counts_out, cfo_abs_err_out, SweepScope{}},
                  SweepOuts{errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out}, flags);
}

extern "C" int ofdm_ber_sweep_task4_ex(ofdm_rx_plan* pl, const void* h, int h_len, int sto_mode, int64_t sto_value,
                                       int cfo_mode, double cfo_value, int time_desync, int freq_desync, int mp_desync,
                                       const double* snr_db, const uint64_t* seeds, int64_t n_points, int64_t frames_per_point,
                                       int64_t frame0, const uint8_t* scr_reg15, int64_t max_frames_per_chunk,
                                       uint64_t* errors_out, uint64_t* status_counts_out, double* cfo_abs_err_out,
                                       uint32_t* frame_errors_out, int64_t mer_skip, double* mer_sums_out,
                                       double* frame_mer_sums_out, int flags) {
  return ofdm_ber_sweep_task4_nmse(pl, h, h_len, sto_mode, sto_value, cfo_mode, cfo_value, time_desync, freq_desync, mp_desync,
                                   snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk,
                                   errors_out, status_counts_out, cfo_abs_err_out, frame_errors_out, mer_skip, mer_sums_out,
                                   frame_mer_sums_out, nullptr, nullptr, flags);
}

extern "C" int ofdm_ber_sweep_task4(ofdm_rx_plan* pl, const void* h, int h_len, int sto_mode, int64_t sto_value, int cfo_mode,
                                    double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                                    const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                                    const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                                    uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                                    int flags) {
  return ofdm_ber_sweep_task4_ex(pl, h, h_len, sto_mode, sto_value, cfo_mode, cfo_value, time_desync, freq_desync, mp_desync,
                                 snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk, errors_out,
                                 status_counts_out, cfo_abs_err_out, frame_errors_out, 0, nullptr, nullptr, flags);
}
