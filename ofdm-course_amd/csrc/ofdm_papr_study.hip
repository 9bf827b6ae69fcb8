// ofdm_papr_study: the PAPR / CCDF study of Task 2 (T2/Main_model_Task_2.m:69-97) over many signals as one device-resident
// call.  A signal is frames_per_signal consecutive generator frames, concatenated (T2:64-68); per chunk of whole signals:
//
//   stage 1  the bit and symbol stages of the fused generator (ofdm_txfused.hip, reused): tx_bits_kernel (Philox payload) or the
//            caller's bits -> [Scrambler per frame, T2:36-51] -> tx_symbols_fused_kernel: the chunk's TX samples in the plan-owned
//            workspace, written once, and the per-symbol sum |x|^2.  No Noise, no channel pass.
//   stage 2  papr_hist_kernel<T, C, TWO_PHASE>: a workgroup owns `window` consecutive window starts of one signal; maximum and
//            sum of every window from the register scans of window_papr_reg_kernel (window_papr_scan, papr_scan.hpp), every value
//            10 log10(max / mean) (calculate_window_PAPR.m:8-14) binned by papr_bin (papr_plan.hpp) into an LDS histogram of
//            uint32 counts; at the end the workgroup adds its non-zero bins and tails to the global uint64 table (64-bit
//            atomicAdd) and folds the maximum |x|^2 of the samples it loaded into the signal's peak (64-bit atomicMax on the bit
//            pattern: non-negative doubles order like unsigned integers).
//            papr_signal_sum_kernel: a signal's sum |x|^2 from its per-symbol partials, in index order.
// HBM: the TX samples written once and read twice (the second time from L2), nothing per window.  Integer counts, an order-free
// maximum and a fixed summation order: every output is independent of the chunking.
//
// Host side: the checks, the chunk and the launch shape are papr_plan.hpp's, plain C++ tested without a GPU.
#include <algorithm>

#include "papr_plan.hpp"
#include "papr_scan.hpp"
#include "txf_generate.hpp"

namespace ofdm {
int tx_bits_device(const ofdm_rx_plan* pl, uint32_t* packed, uint8_t* bits, uint32_t k0, uint32_t k1, uint32_t stream0,
                   int64_t nf);                                          // ofdm_txgen.hip

// |x|^2 as round(round(re^2) + round(im^2)): the products are kept from fusing into the sum, so that the peak is the double a
// host computes from the returned samples
template <typename T>
__device__ __forceinline__ double power_unfused(cx<T> v) {
  double a = (double)v.x * (double)v.x, b = (double)v.y * (double)v.y;
  asm volatile("" : "+v"(a), "+v"(b));
  return a + b;
}

// grid = (workgroups per signal, signals of the chunk); dynamic LDS = scan_doubles doubles, then n_bins + PAPR_TAILS uint32
//   tx: the chunk's signals, signal_samples each; n_out = signal_samples - W + 1 windows per signal
//   hist [n_bins], tails [PAPR_TAILS]: the call's tables; signal (optional): [signals of the chunk][2], [0] = the peak
template <typename T, int C, bool TWO_PHASE>
__global__ void papr_hist_kernel(const cx<T>* __restrict__ tx, int64_t signal_samples, int W, int64_t n_out, int scan_doubles,
                                 int n_bins, double lo_db, double hi_db, unsigned long long* __restrict__ hist,
                                 unsigned long long* __restrict__ tails, double* __restrict__ signal) {
  extern __shared__ double a[];
  __shared__ double wtot_m[16], wtot_s[16];
  uint32_t* const cnt = (uint32_t*)(a + scan_doubles);
  const int nt = blockDim.x, tid = threadIdx.x;
  for (int i = tid; i < n_bins + PAPR_TAILS; i += nt) cnt[i] = 0u;          // (the scan synchronises before its first emit)
  const cx<T>* x = tx + (int64_t)blockIdx.y * signal_samples;
  double pk = 0.0;
  window_papr_scan<T, C, TWO_PHASE>(x, signal_samples, W, (int64_t)blockIdx.x * W, n_out, a, wtot_m, wtot_s,
                                    [&](int64_t, double v) { atomicAdd(&cnt[papr_bin(v, lo_db, hi_db, n_bins)], 1u); },
                                    [&](cx<T> s) { pk = fmax(pk, power_unfused(s)); });
  __syncthreads();
  for (int i = tid; i < n_bins + PAPR_TAILS; i += nt) {
    const uint32_t c = cnt[i];
    if (c) atomicAdd(i < n_bins ? hist + i : tails + (i - n_bins), (unsigned long long)c);
  }
  if (signal) {
#pragma unroll
    for (int d = 32; d; d >>= 1) pk = fmax(pk, __shfl_xor(pk, d, 64));
    if ((tid & 63) == 0 && pk > 0.0)
      atomicMax((unsigned long long*)(signal + 2 * (int64_t)blockIdx.y), (unsigned long long)__double_as_longlong(pk));
  }
}

// signal[s][1] = the sum |x|^2 of signal s: its per_signal per-symbol partials (tx_symbols_fused_kernel) in index order
__global__ __launch_bounds__(256) void papr_signal_sum_kernel(const double* __restrict__ partial, int64_t per_signal, int64_t n_signals,
                                                              double* __restrict__ signal) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= n_signals) return;
  double sum = 0.0;
  for (int64_t i = 0; i < per_signal; ++i) sum += partial[s * per_signal + i];
  signal[2 * s + 1] = sum;
}

template <typename T>
static int launch_hist(const PaprPass& p, const void* tx, int64_t signal_samples, int window, int n_bins, double lo_db,
                       double hi_db, unsigned long long* hist, unsigned long long* tails, double* signal) {
  auto launch = [&](auto kern) -> int {
    OFDM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
    hipLaunchKernelGGL(kern, dim3(p.grid_x, p.grid_y), dim3(p.threads), p.lds, ctx().stream, (const cx<T>*)tx, signal_samples,
                       window, p.windows, (int)(p.scan_bytes / sizeof(double)), n_bins, lo_db, hi_db, hist, tails, signal);
    return check_launch("papr_hist_kernel");
  };
  if (p.per_thread == 4) return launch(papr_hist_kernel<T, 4, false>);
  if (p.per_thread == 8) return launch(papr_hist_kernel<T, 8, false>);
  return launch(papr_hist_kernel<T, 16, true>);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_papr_study(ofdm_rx_plan* pl, uint64_t seed, int64_t frame0, int64_t n_signals, int frames_per_signal,
                               const uint8_t* scr_reg15, const uint8_t* payload_bits, int window, int n_bins, double lo_db,
                               double hi_db, int64_t max_frames_per_chunk, uint64_t* hist_out, uint64_t* tails_out,
                               double* signal_out, void* tx_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  PaprCall c;
  c.plan = pl ? &s : nullptr;
  c.out = hist_out && tails_out;
  c.f64_flag = is_f64(flags);
  c.frame0 = frame0; c.n_signals = n_signals; c.frames_per_signal = frames_per_signal;
  c.scr_reg15 = scr_reg15;
  c.window = window; c.n_bins = n_bins; c.lo_db = lo_db; c.hi_db = hi_db;
  c.max_chunk = max_frames_per_chunk;
  PaprWhy why;
  if (const int id = papr_prelude(c, why)) {
    set_error("%s", why.text);
    return id == PAPR_REFUSE_DEVICE ? OFDM_ERR_STATE : OFDM_ERR_ARG;
  }
  const size_t cs = csize(flags);
  const int64_t frame_samples = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const int64_t signal_samples = frame_samples * frames_per_signal;
  const int64_t frame_bits = (int64_t)pl->nd * pl->n_symb * pl->bps;
  const int64_t n_frames = n_signals * frames_per_signal;
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  void *dhist, *dtails, *dsignal, *dtx;
  const void* dbits;
  OFDM_TRY(st.out(hist_out, sizeof(uint64_t) * (size_t)n_bins, &dhist));
  OFDM_TRY(st.out(tails_out, sizeof(uint64_t) * PAPR_TAILS, &dtails));
  OFDM_TRY(st.out(signal_out, sizeof(double) * 2 * (size_t)n_signals, &dsignal));
  OFDM_TRY(st.out(tx_out, cs * (size_t)signal_samples * n_signals, &dtx));
  OFDM_TRY(st.in(payload_bits, (size_t)frame_bits * n_frames, &dbits));
  OFDM_HIP(hipMemsetAsync(dhist, 0, sizeof(uint64_t) * (size_t)n_bins, stream));         // overwritten, not accumulated
  OFDM_HIP(hipMemsetAsync(dtails, 0, sizeof(uint64_t) * PAPR_TAILS, stream));
  if (dsignal && n_signals) OFDM_HIP(hipMemsetAsync(dsignal, 0, sizeof(double) * 2 * (size_t)n_signals, stream));
  if (n_signals == 0) return st.finish();
  OFDM_TRY(tx_dict_device(pl));
  const bool scr = scr_reg15 != nullptr;
  const int64_t CS = papr_chunk_signals(s, scr, n_signals, frames_per_signal, max_frames_per_chunk);
  TxfBuffers b;
  OFDM_TRY(txf_workspace(pl, CS * frames_per_signal, papr_use(scr), b));
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int64_t s0 = 0; s0 < n_signals; s0 += CS) {
    const int64_t ns = std::min<int64_t>(CS, n_signals - s0);
    const int64_t f0 = s0 * frames_per_signal, nf = ns * frames_per_signal;
    const uint32_t stream0 = (uint32_t)(frame0 + f0);
    const uint8_t* given = dbits ? (const uint8_t*)dbits + frame_bits * f0 : nullptr;
    const uint8_t* sc = given;                                    // Scrambler off: the symbol kernel reads the caller's bits
    if (scr) {                                                    // Scrambler.m per frame, register reset (T2:36-51)
      if (given) OFDM_HIP(hipMemcpyAsync(b.b0, given, (size_t)frame_bits * nf, hipMemcpyDeviceToDevice, stream));
      else OFDM_TRY(tx_bits_device(pl, nullptr, b.b0, k0, k1, stream0, nf));
      OFDM_TRY(ofdm_Scrambler_frames(scr_reg15, b.b0, frame_bits, nf, b.b1, OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0)));
      sc = b.b1;
    }
    OFDM_TRY(txf_symbols(pl, b.tx, b.partial, sc, k0, k1, stream0, nf));
    double* sig = dsignal ? (double*)dsignal + 2 * s0 : nullptr;
    const PaprPass p = papr_pass(window, n_bins, signal_samples, ns);
    if (pl->f64)
      OFDM_TRY(launch_hist<double>(p, b.tx, signal_samples, window, n_bins, lo_db, hi_db, (unsigned long long*)dhist,
                                   (unsigned long long*)dtails, sig));
    else
      OFDM_TRY(launch_hist<float>(p, b.tx, signal_samples, window, n_bins, lo_db, hi_db, (unsigned long long*)dhist,
                                  (unsigned long long*)dtails, sig));
    if (sig) {
      hipLaunchKernelGGL(papr_signal_sum_kernel, dim3(cdiv_u(ns, 256)), dim3(256), 0, stream, (const double*)b.partial,
                         (int64_t)frames_per_signal * pl->n_symb, ns, sig);
      OFDM_TRY(check_launch("papr_signal_sum_kernel"));
    }
    if (dtx)
      OFDM_HIP(hipMemcpyAsync((unsigned char*)dtx + cs * (size_t)signal_samples * s0, b.tx, cs * (size_t)signal_samples * ns,
                              hipMemcpyDeviceToDevice, stream));
  }
  return st.finish();
}
