// ofdm_tx_frames_fused / ofdm_ber_sweep_task5: the reference-order frame generator in three sample passes, and one
// device-resident tile of a BER(SNR) sweep on top of it (T3/Main_model_Task_3.m:237-268, T5/Task5_part2.m:134,:148-152).
//
// Per frame (T5/Main_model_Task_5.m:50-127, Noise.m:3-10):
//   payload -> [Scrambler per frame] -> mapping -> OFDM_map_carriers -> OFDM_modulator -> Noise(snr_db) -> conv(h) truncated
// with the draws of ofdm_tx_frames_ex(noise_first = 1): payload Philox (seed, frame0 + f), noise Philox counter
// (i, 0, frame0 + f, 0) through awgn_kernel's Box-Muller, per-frame noise power from the frame's own mean |x|^2.
//
//   tx_symbols_fused_kernel<T, N>   one transform per symbol (the wg_fft of mod_kernel): the carriers are built in registers
//                                   from the plan's role tables and the payload draw (no X buffer), 1/N, symbol + CP written
//                                   once, and the symbol's sum |x|^2 (CP included, double) into partial[frame][symbol].
//   tx_channel_fused_kernel<T>      one workgroup per (segment of TXF_SEG samples, frame): sigma from the frame's partials
//                                   (fixed order, no atomics), segment + halo of max_delay samples loaded into LDS with the
//                                   noise added (the halo's noise is regenerated: it is a pure function of the counter),
//                                   the sparse FIR from LDS with the taps in kernel arguments, rx written once (nontemporal).
//   ber_point_reduce_kernel         per-frame uint32 errors -> per-point uint64 (integers: exact in any order).
// TX samples: one write, one read (+ halo), RX: one write -- 3 sample passes against ~9 for ofdm_tx_frames_ex's stages.
//
// ofdm_tx_frames_fused_ex / ofdm_ber_sweep_task4 add the Task-4 impairments (T4/Main_model_Task_4.m:99-110, add_STO.m,
// add_CFO.m) in the reference order Noise -> add_STO -> add_CFO -> conv, still in three sample passes:
//   tx_channel_imp_kernel<T>        tx_channel_fused_kernel's body (tx_channel_body) with IMP on: its LDS load stage builds
//                                   z[m] = w[m + sto_f] e^{2 pi i cfo_f m / Nfft} for the segment and its halo, the noise of w
//                                   drawn at the SOURCE index m + sto_f (Noise comes before the shift).  The shift is uniform
//                                   per frame: no extra halo, the loads stay coalesced.
//   t4_point_reduce_kernel          per-frame errors / status / |FreqOffset + IFO - Freq_Shift| of a whole point -> its sums,
//                                   in a fixed order (the double sum does not depend on the chunking).
//   t4_point_mer_kernel             per-frame MER_func sums -> per-point sums in the same fixed order (both sweeps with MER).
// The per-frame draws are tx_draw_kernel's (ofdm_txgen.hip), the draws of ofdm_tx_frames_ex.
//
// ofdm_tx_frames_fading / ofdm_ber_sweep_task5_fading draw a channel per frame (the Monte-Carlo realisations of
// T5/Task5_part2.m:148-155) on one tap-delay line, still in three sample passes:
//   tx_fade_draw_kernel             tap t of frame f: a = g_t e^{2 pi i u}, u from Philox counter (t, 0, frame0 + f, 3), double
//   tx_channel_fade_kernel<T>       tx_channel_body with FADE on: the delays and the halo stay in the kernel arguments (uniform
//                                   over the launch), the amplitudes of frame blockIdx.y are read once per workgroup into the
//                                   tail of the dynamic LDS, cast to T as the static path casts h
//   t5_frame_nmse_kernel<T>         one workgroup per frame: H_f(k) = sum_t a_t e^{-2 pi i d_t k / Nfft} in double (the phase
//                                   d_t k mod Nfft reduced in integers), sum_k |H_f(k) - Hest_f(k)|^2 over 1..N_carrier in a
//                                   fixed order (T5/Task5_part2.m:202-205); the points through t4_point_mer_kernel<1>
//
// ofdm_tx_frames_fading_ex / ofdm_ber_sweep_task4_fading / ofdm_ber_sweep_task4_nmse put both together for the Task-4 receiver
// (T4/Main_model_Task_4.m:94-110,:257-267 over the realisations of T5/Task5_part2.m:148-155, NMSE of T4:205-239):
//   tx_channel_imp_fade_kernel<T>   tx_channel_body with IMP and FADE on: the load stage is tx_channel_imp_kernel's (Noise ->
//                                   add_STO -> add_CFO), the frame's amplitudes staged behind the segment as in
//                                   tx_channel_fade_kernel; the two per-frame draws stay independent (counter word 3 = 2 / 3)
//   tx_static_amp_kernel            the static channel's taps into device memory once per sweep, so that t5_frame_nmse_kernel
//                                   reads them with a frame stride of 0
//
// Host side: both generator entries forward to one body (txf_frames); given impairments it launches the draw kernel and
// tx_channel_imp_kernel, else tx_channel_fused_kernel.  The two sweeps share their common checks and outputs
// (txf_check_sweep, txf_sweep_outputs), the point x chunk loop with the generation inside (txf_sweep_points, the receiver
// passed as a callable) and the MER reduction (txf_point_mer); each keeps its own outputs, scratch, chunk budget and
// per-point reduction.  The fading entries share those bodies: txf_frames / txf_sweep_points given a TxfFade launch
// tx_fade_draw_kernel and tx_channel_fade_kernel (tx_channel_imp_fade_kernel given impairments too), both Task-5 sweep entries
// forward to t5_sweep and the Task-4 sweep entries to t4_sweep.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "fft_core.hpp"
#include "rx_plan.hpp"
#include "t4_route.hpp"
#include "tx_philox.hpp"

namespace ofdm {
int tx_dict_device(ofdm_rx_plan* pl);                                                       // ofdm_txgen.hip
int tx_bits_device(const ofdm_rx_plan* pl, uint32_t* packed, uint8_t* bits, uint32_t k0, uint32_t k1, uint32_t stream0,
                   int64_t nf);
int tx_pack_bits_device(const ofdm_rx_plan* pl, const uint8_t* bits, uint32_t* packed, int64_t nf);
int tx_draw_device(const ofdm_rx_plan* pl, int64_t* sto, double* cfo, int sto_mode, int64_t sto_value, int cfo_mode,
                   double cfo_value, uint32_t k0, uint32_t k1, uint32_t stream0, int64_t nf);

constexpr int TXF_MAX_TAPS = 64;
constexpr int TXF_MAX_DELAY = 4096;
constexpr int TXF_SEG = 4096;                       // output samples per channel workgroup
constexpr size_t TXF_WS_BUDGET = size_t(2) << 30;   // chunk cap of the plan-owned workspace

template <typename T>
struct TxfTaps {
  int32_t delay[TXF_MAX_TAPS];
  cx<T> amp[TXF_MAX_TAPS];
  int n;
  int halo;                                          // largest delay: samples before a segment the FIR reaches back to
};

// ---------------------------------------------------------------------------------------------
// map_carriers + OFDM_modulator of one symbol per transform, carriers from the role tables
// ---------------------------------------------------------------------------------------------
template <typename T, int N>
__global__ __launch_bounds__(fft_wg_threads(N)) void tx_symbols_fused_kernel(
    cx<T>* __restrict__ tx, double* __restrict__ partial, const cx<T>* __restrict__ tw, const int16_t* __restrict__ prole,
    const int16_t* __restrict__ drole, const cx<T>* __restrict__ pilots, const cx<T>* __restrict__ dict,
    const uint8_t* __restrict__ sc_bits, int n_symb, int t_guard, int nd, int bps, uint32_t k0, uint32_t k1,
    uint32_t stream0, int64_t n_sym_total) {
  constexpr int TPX = N / 8;
  constexpr int XPW = fft_xforms_per_wg(N);
  __shared__ cx<T> lds[XPW * fft_lds_elems(N)];
  const int g = threadIdx.x / TPX;
  const int j = threadIdx.x % TPX;
  const int64_t q = (int64_t)blockIdx.x * XPW + g;              // symbol of the chunk, frame-major
  const bool live = q < n_sym_total;
  const int64_t f = live ? q / n_symb : 0;
  const int s = live ? (int)(q - f * n_symb) : 0;
  const int64_t frame_bits = (int64_t)nd * n_symb * bps;
  cx<T> v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = j + e * TPX;
    const int p = prole[k], d = drole[k];
    cx<T> val = mk<T>(0, 0);
    if (live) {
      if (p >= 0) val = pilots[p];                               // pilot rows written last in OFDM_map_carriers.m:8
      else if (d >= 0) {
        uint32_t code;
        if (sc_bits) {                                           // the frame's scrambled bits, bps per symbol, MSB first
          const uint8_t* b = sc_bits + f * frame_bits + ((int64_t)s * nd + d) * bps;
          code = 0;
          for (int r = 0; r < bps; ++r) code = (code << 1) | (uint32_t)(b[r] & 1u);
        } else {
          code = payload_code((uint64_t)s * nd + d, stream0 + (uint32_t)f, k0, k1, bps);
        }
        val = dict[code];
      }
    }
    v[e] = val;
  }
  wg_fft<T, N, true>(v, j, tw, lds + g * fft_lds_elems(N));
  double ps = 0;
  if (live) {
    const T scale = T(1) / T(N);
    cx<T>* dst = tx + q * (int64_t)(N + t_guard);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int idx = j + e * TPX;
      const cx<T> val = v[e] * scale;
      const double e2 = (double)val.x * (double)val.x + (double)val.y * (double)val.y;
      dst[t_guard + idx] = val;
      ps += e2;
      if (idx >= N - t_guard) {                                  // OFDM_modulator.m:8-9
        dst[idx - (N - t_guard)] = val;
        ps += e2;
      }
    }
  }
  // the symbol's sum: butterfly inside the transform's lanes (a fixed order), then the waves of a multi-wave transform
  constexpr int W = TPX < 64 ? TPX : 64;
#pragma unroll
  for (int off = W / 2; off > 0; off >>= 1) ps += __shfl_xor(ps, off, 64);
  if constexpr (TPX <= 64) {
    if (j == 0 && live) partial[q] = ps;
  } else {
    constexpr int NWV = TPX / 64;                                // waves per transform (N = 1024: two transforms of two)
    __shared__ double wsum[XPW * NWV];
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ps;
    __syncthreads();
    if (j == 0 && live) {
      double t = 0;
      for (int w = 0; w < NWV; ++w) t += wsum[g * NWV + w];
      partial[q] = t;
    }
  }
}

// x + sigma * (n_re + i n_im): awgn_kernel's Box-Muller on the same Philox words, in the same arithmetic per precision
template <typename T>
__device__ __forceinline__ cx<T> txf_noisy(cx<T> v, int64_t i, double sg, uint32_t stream, uint32_t k0, uint32_t k1) {
  uint32_t r[4];
  philox_words((uint32_t)i, (uint32_t)((uint64_t)i >> 32), stream, 0u, k0, k1, r);
  const double u0 = ((double)r[0] + 0.5) * 2.3283064365386963e-10;
  const double u1 = ((double)r[1] + 0.5) * 2.3283064365386963e-10;
  if constexpr (std::is_same<T, float>::value) {
    const float rad = sqrtf(-2.0f * logf((float)u0)) * (float)sg;
    float sn, cs;
    sincospif((float)(2.0 * u1), &sn, &cs);
    return mk<T>(v.x + rad * cs, v.y + rad * sn);
  } else {
    const double rad = sqrt(-2.0 * log(u0));
    double sn, cs;
    sincospi(2.0 * u1, &sn, &cs);
    return mk<T>((T)((double)v.x + sg * rad * cs), (T)((double)v.y + sg * rad * sn));
  }
}

// ---------------------------------------------------------------------------------------------
// Noise (Noise.m:3-10) then conv(h) truncated per frame (T5/Task5_part2.m:152), one segment per workgroup.
// grid = (segments, frames); dynamic LDS = (TXF_SEG + halo) samples.
// IMP adds add_STO -> add_CFO between Noise and conv (T4/Main_model_Task_4.m:99-110,:257-267), folded into the LDS load
// stage with the frame's shift sto[f] and rotation cfo[f]:
//   w[j] = x[j] + sigma n(j)   s[m] = w[m + sto] (0 outside the frame, add_STO.m, either sign)
//   z[m] = s[m] exp(2 pi i cfo m / Nfft)   (add_CFO.m on the shifted stream; the arithmetic of sto_cfo_frames_kernel)
// ---------------------------------------------------------------------------------------------
// FADE: the taps' amplitudes are those of the frame, famp[f][taps.n] (complex double, tx_fade_draw_kernel), staged behind the
// segment in LDS; taps.amp is not read.
template <typename T, bool IMP, bool FADE = false>
__device__ __forceinline__ void tx_channel_body(const cx<T>* __restrict__ tx, cx<T>* __restrict__ rx,
                                                const double* __restrict__ partial, int n_symb, int64_t len, double snr_lin,
                                                uint32_t k0, uint32_t k1, uint32_t stream0, const int64_t* __restrict__ sto,
                                                const double* __restrict__ cfo, double inv_nfft, const TxfTaps<T>& taps,
                                                const c64* __restrict__ famp = nullptr) {
  extern __shared__ __attribute__((aligned(16))) unsigned char txf_smem[];
  cx<T>* buf = (cx<T>*)txf_smem;
  const int64_t f = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * TXF_SEG;
  const int H = taps.halo;
  const cx<T>* x = tx + f * len;
  double sum = 0;                                                // Noise.m:3 -- the frame's symbols in order
  for (int i = 0; i < n_symb; ++i) sum += partial[f * n_symb + i];
  const double sg = sqrt(sum / (double)len / snr_lin / 2.0);     // :5, per-component sigma
  const uint32_t stream = stream0 + (uint32_t)f;
  int64_t sh = 0;                                                // uniform per frame: no extra halo, coalesced loads
  double fo = 0.0;
  if constexpr (IMP) {
    sh = sto[f];
    fo = cfo[f];
  }
  for (int i = threadIdx.x; i < TXF_SEG + H; i += 256) {
    const int64_t m = n0 - H + i;                                // index of the shifted stream; before the frame: silence
    const int64_t src = m + sh;
    cx<T> v = mk<T>(0, 0);
    if (m >= 0 && m < len && src >= 0 && src < len) {
      v = txf_noisy<T>(x[src], src, sg, stream, k0, k1);         // the noise of the source sample (Noise before add_STO)
      if constexpr (IMP) {
        if (fo != 0.0) {                                         // cfo 0: a rotation by exactly 1, skipped (uniform per frame)
          const double t = fo * (double)m * inv_nfft;
          const double fr = t - floor(t);
          double sn, cs;
          sincospi(2.0 * fr, &sn, &cs);
          v = mk<T>((T)((double)v.x * cs - (double)v.y * sn), (T)((double)v.x * sn + (double)v.y * cs));
        }
      }
    }
    buf[i] = v;
  }
  cx<T>* fa = buf + TXF_SEG + H;                                 // FADE: the frame's amplitudes, read once per workgroup
  if constexpr (FADE) {
    if ((int)threadIdx.x < taps.n) {
      const c64 a = famp[f * taps.n + threadIdx.x];
      fa[threadIdx.x] = mk<T>((T)a.x, (T)a.y);
    }
  }
  __syncthreads();
  cx<T>* y = rx + f * len;
  for (int o = threadIdx.x; o < TXF_SEG; o += 256) {
    if (n0 + o >= len) break;
    cx<T> acc = mk<T>(0, 0);
    if constexpr (FADE) {
      for (int t = 0; t < taps.n; ++t) acc = acc + buf[H + o - taps.delay[t]] * fa[t];
    } else {
      for (int t = 0; t < taps.n; ++t) acc = acc + buf[H + o - taps.delay[t]] * taps.amp[t];
    }
    nt_store(y + n0 + o, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tx_channel_fused_kernel(const cx<T>* __restrict__ tx, cx<T>* __restrict__ rx,
                                                               const double* __restrict__ partial, int n_symb, int64_t len,
                                                               double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0,
                                                               TxfTaps<T> taps) {
  tx_channel_body<T, false>(tx, rx, partial, n_symb, len, snr_lin, k0, k1, stream0, nullptr, nullptr, 0.0, taps);
}

template <typename T>
__global__ __launch_bounds__(256) void tx_channel_imp_kernel(const cx<T>* __restrict__ tx, cx<T>* __restrict__ rx,
                                                             const double* __restrict__ partial, int n_symb, int64_t len,
                                                             double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0,
                                                             const int64_t* __restrict__ sto, const double* __restrict__ cfo,
                                                             double inv_nfft, TxfTaps<T> taps) {
  tx_channel_body<T, true>(tx, rx, partial, n_symb, len, snr_lin, k0, k1, stream0, sto, cfo, inv_nfft, taps);
}

// dynamic LDS = (TXF_SEG + halo + taps.n) samples
template <typename T>
__global__ __launch_bounds__(256) void tx_channel_fade_kernel(const cx<T>* __restrict__ tx, cx<T>* __restrict__ rx,
                                                              const double* __restrict__ partial, int n_symb, int64_t len,
                                                              double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0,
                                                              const c64* __restrict__ famp, TxfTaps<T> taps) {
  tx_channel_body<T, false, true>(tx, rx, partial, n_symb, len, snr_lin, k0, k1, stream0, nullptr, nullptr, 0.0, taps, famp);
}

// IMP and FADE: add_STO -> add_CFO of the frame's draws between Noise and the conv with the frame's own amplitudes
// (T4/Main_model_Task_4.m:94-110,:257-267 per realisation of T5/Task5_part2.m:148-155); dynamic LDS as tx_channel_fade_kernel
template <typename T>
__global__ __launch_bounds__(256) void tx_channel_imp_fade_kernel(const cx<T>* __restrict__ tx, cx<T>* __restrict__ rx,
                                                                  const double* __restrict__ partial, int n_symb, int64_t len,
                                                                  double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0,
                                                                  const int64_t* __restrict__ sto,
                                                                  const double* __restrict__ cfo, double inv_nfft,
                                                                  const c64* __restrict__ famp, TxfTaps<T> taps) {
  tx_channel_body<T, true, true>(tx, rx, partial, n_symb, len, snr_lin, k0, k1, stream0, sto, cfo, inv_nfft, taps, famp);
}

// per-frame channel draw, the sibling of tx_draw_kernel: tap t of frame f is gain[t] (cospi(2u) + i sinpi(2u)) with
// u = (word0 + 0.5) 2^-32 of Philox counter (t, 0, stream0 + f, 3) -- static taps with random initial phases, the stand-in
// for lteFadingChannel of drivers/common.py:fading_taps drawn on the device.  amp / taps_out: [n_frames][n_taps].
struct TxfGains {
  double g[TXF_MAX_TAPS];
};

__global__ __launch_bounds__(256) void tx_fade_draw_kernel(c64* __restrict__ amp, c64* __restrict__ taps_out, TxfGains gains,
                                                           int n_taps, uint32_t k0, uint32_t k1, uint32_t stream0,
                                                           int64_t n_frames) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_frames * n_taps) return;
  const int64_t f = i / n_taps;
  const int t = (int)(i - f * n_taps);
  uint32_t r[4];
  philox_words((uint32_t)t, 0u, stream0 + (uint32_t)f, 3u, k0, k1, r);
  const double u = ((double)r[0] + 0.5) * 2.3283064365386963e-10;
  double sn, cs;
  sincospi(2.0 * u, &sn, &cs);
  const c64 a{gains.g[t] * cs, gains.g[t] * sn};
  amp[i] = a;
  if (taps_out) taps_out[i] = a;
}

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
// amp_stride: dl.n for the amplitudes of a channel per frame [frames][dl.n], 0 for one static channel [dl.n].
struct TxfDelays {
  int32_t d[TXF_MAX_TAPS];
  int n;
};

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
    double hr = 0, hi = 0;
    for (int t = 0; t < dl.n; ++t) {
      const int m = (int)(((int64_t)dl.d[t] * k) % nfft);       // the phase reduced in integers: the argument stays in [0, 2)
      double sn, cs;
      sincospi((double)m * inv, &sn, &cs);
      hr += a[t].x * cs + a[t].y * sn;                           // a (cs - i sn)
      hi += a[t].y * cs - a[t].x * sn;
    }
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
struct TxfChannel {                                  // nonzero taps of h (conv_common's rule: exact zeros are skipped)
  std::vector<int32_t> delay;
  std::vector<c64> amp;
  int halo = 0;
};

static int txf_channel(const void* h, int h_len, bool f64, TxfChannel& ch) {
  OFDM_ARG(h_len >= 0 && (h || h_len == 0), "tx_frames_fused: bad channel");
  if (!h || h_len == 0) {                            // no channel: one unit tap (x * (1 + 0i) is exact)
    ch.delay.assign(1, 0);
    ch.amp.assign(1, c64{1.0, 0.0});
    return OFDM_OK;
  }
  for (int d = 0; d < h_len; ++d) {
    const double re = f64 ? ((const c64*)h)[d].x : ((const c32*)h)[d].x;
    const double im = f64 ? ((const c64*)h)[d].y : ((const c32*)h)[d].y;
    if (re != 0.0 || im != 0.0) {
      OFDM_ARG(d <= TXF_MAX_DELAY, "tx_frames_fused: channel tap at delay %d (at most %d)", d, TXF_MAX_DELAY);
      ch.delay.push_back(d);
      ch.amp.push_back(c64{re, im});
      ch.halo = d;
    }
  }
  OFDM_ARG((int)ch.delay.size() <= TXF_MAX_TAPS, "tx_frames_fused: %d nonzero channel taps (at most %d)",
           (int)ch.delay.size(), TXF_MAX_TAPS);
  return OFDM_OK;
}

// a per-frame channel on one tap-delay line: ch.delay / ch.halo as for a static h, the amplitudes drawn per chunk
struct TxfFade {
  TxfGains gains;                                    // g_t = sqrt(tap_power[t] / sum tap_power), double
  c64* amp = nullptr;                                // the chunk's amplitudes [nf][n_taps] (tx_fade_draw_kernel)
  c64* taps_out = nullptr;                           // generator: where the caller wants them (optional)
};

static int txf_fading(const int32_t* tap_delay, const double* tap_power, int n_taps, const char* what, TxfChannel& ch,
                      TxfFade& fd) {
  OFDM_ARG(n_taps >= 1 && n_taps <= TXF_MAX_TAPS, "%s: n_taps must be 1 .. %d", what, TXF_MAX_TAPS);
  OFDM_ARG(tap_delay && tap_power, "%s: tap_delay / tap_power missing", what);
  double total = 0;
  for (int t = 0; t < n_taps; ++t) {
    OFDM_ARG(tap_delay[t] >= 0 && tap_delay[t] <= TXF_MAX_DELAY, "%s: tap delay %d outside 0 .. %d", what, tap_delay[t],
             TXF_MAX_DELAY);
    for (int q = 0; q < t; ++q) OFDM_ARG(tap_delay[q] != tap_delay[t], "%s: tap delay %d given twice", what, tap_delay[t]);
    OFDM_ARG(tap_power[t] > 0.0 && std::isfinite(tap_power[t]), "%s: tap powers must be positive and finite", what);
    total += tap_power[t];
  }
  OFDM_ARG(std::isfinite(total), "%s: tap powers must be positive and finite", what);
  fd.gains = TxfGains{};
  for (int t = 0; t < n_taps; ++t) {
    fd.gains.g[t] = std::sqrt(tap_power[t] / total);
    ch.delay.push_back(tap_delay[t]);
    ch.amp.push_back(c64{fd.gains.g[t], 0.0});
    ch.halo = std::max(ch.halo, (int)tap_delay[t]);
  }
  return OFDM_OK;
}

template <typename T>
static TxfTaps<T> txf_taps(const TxfChannel& ch) {
  TxfTaps<T> tp{};
  tp.n = (int)ch.delay.size();
  tp.halo = ch.halo;
  for (int t = 0; t < tp.n; ++t) {
    tp.delay[t] = ch.delay[t];
    tp.amp[t] = mk<T>((T)ch.amp[t].x, (T)ch.amp[t].y);
  }
  return tp;
}

template <typename T, int N>
static int launch_symbols(const ofdm_rx_plan* pl, const void* tw, void* tx, double* partial, const uint8_t* sc_bits,
                          uint32_t k0, uint32_t k1, uint32_t stream0, int64_t nf) {
  constexpr int XPW = fft_xforms_per_wg(N);
  const int64_t n_sym = (int64_t)pl->n_symb * nf;
  hipLaunchKernelGGL((tx_symbols_fused_kernel<T, N>), dim3(cdiv_u(n_sym, XPW)), dim3(fft_wg_threads(N)), 0, ctx().stream,
                     (cx<T>*)tx, partial, (const cx<T>*)tw, (const int16_t*)pl->d_prole, (const int16_t*)pl->d_drole,
                     (const cx<T>*)pl->d_pilots, (const cx<T>*)pl->d_dict, sc_bits, pl->n_symb, pl->t_guard, pl->nd, pl->bps,
                     k0, k1, stream0, n_sym);
  return check_launch("tx_symbols_fused_kernel");
}

// the Task-4 impairments of a generator call (T4/Main_model_Task_4.m:99-110): modes 0 off, 1 fixed, 2 drawn; the chunk's
// per-frame draws are written to sto / cfo (nf entries each)
struct TxfImp {
  int sto_mode = 0;
  int64_t sto_value = 0;
  int cfo_mode = 0;
  double cfo_value = 0;
  int64_t* sto = nullptr;
  double* cfo = nullptr;
};

// fade (optional): tx_channel_fade_kernel with the chunk's amplitudes fade->amp;
// imp (optional): tx_channel_imp_kernel with the chunk's draws imp->sto / imp->cfo; both: tx_channel_imp_fade_kernel;
// neither: tx_channel_fused_kernel
template <typename T>
static int launch_channel(const ofdm_rx_plan* pl, const TxfChannel& ch, const void* tx, void* rx, const double* partial,
                          double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0, const TxfImp* imp, const TxfFade* fade,
                          int64_t nf) {
  const int64_t len = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t dyn = sizeof(cx<T>) * (size_t)(TXF_SEG + ch.halo + (fade ? ch.delay.size() : 0));
  const dim3 grid(cdiv_u(len, TXF_SEG), (unsigned)nf);
  const void* kernel = fade ? (imp ? (const void*)tx_channel_imp_fade_kernel<T> : (const void*)tx_channel_fade_kernel<T>)
                            : imp ? (const void*)tx_channel_imp_kernel<T> : (const void*)tx_channel_fused_kernel<T>;
  // > 64 KB for long channels: the attribute is per device, so it is set on every launch (not cached per process)
  OFDM_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  if (fade && imp) {
    hipLaunchKernelGGL(tx_channel_imp_fade_kernel<T>, grid, dim3(256), dyn, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                       pl->n_symb, len, snr_lin, k0, k1, stream0, imp->sto, imp->cfo, 1.0 / (double)pl->nfft,
                       (const c64*)fade->amp, txf_taps<T>(ch));
    return check_launch("tx_channel_imp_fade_kernel");
  }
  if (fade) {
    hipLaunchKernelGGL(tx_channel_fade_kernel<T>, grid, dim3(256), dyn, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                       pl->n_symb, len, snr_lin, k0, k1, stream0, (const c64*)fade->amp, txf_taps<T>(ch));
    return check_launch("tx_channel_fade_kernel");
  }
  if (imp)
    hipLaunchKernelGGL(tx_channel_imp_kernel<T>, grid, dim3(256), dyn, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                       pl->n_symb, len, snr_lin, k0, k1, stream0, imp->sto, imp->cfo, 1.0 / (double)pl->nfft, txf_taps<T>(ch));
  else
    hipLaunchKernelGGL(tx_channel_fused_kernel<T>, grid, dim3(256), dyn, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                       pl->n_symb, len, snr_lin, k0, k1, stream0, txf_taps<T>(ch));
  return check_launch(imp ? "tx_channel_imp_kernel" : "tx_channel_fused_kernel");
}

// chunk buffers inside the plan-owned workspace
struct TxfBuffers {
  void* tx = nullptr;
  double* partial = nullptr;
  uint8_t* b0 = nullptr;                             // Scrambler on: payload bits, one byte each
  uint8_t* b1 = nullptr;                             // Scrambler on: scrambled bits
  void* rx = nullptr;                                // sweep: the chunk's RX frames
  uint32_t* ref = nullptr;                           // sweep: their packed reference bits
  int64_t* sto = nullptr;                            // impairments on: the chunk's draws
  double* cfo = nullptr;
  c64* amp = nullptr;                                // fading: the chunk's tap amplitudes [ch][n_taps]
  void* hest = nullptr;                              // sweep with NMSE: the chunk's channel estimates [N_carrier x ch]
};

// what a call adds to the plain generator workspace
struct TxfExtras {
  bool imp = false;                                  // the Task-4 impairment draws
  int fade_taps = 0;                                 // > 0: a per-frame channel of that many taps
  bool hest = false;                                 // the receiver's channel estimates (sweep)
};

static size_t a256(size_t b) { return (b + 255) & ~size_t(255); }

static size_t txf_frame_bytes(const ofdm_rx_plan* pl, bool scr, bool sweep, const TxfExtras& x = TxfExtras()) {
  const size_t cs = pl->f64 ? sizeof(c64) : sizeof(c32);
  const size_t fs = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t frame_bits = (size_t)pl->nd * pl->n_symb * pl->bps;
  return cs * fs * (sweep ? 2 : 1) + 8 * (size_t)pl->n_symb + (scr ? 2 * frame_bits : 0) +
         (sweep ? (size_t)pl->frame_words * 4 : 0) + (x.imp ? 16 : 0) + sizeof(c64) * (size_t)x.fade_taps +
         (x.hest ? cs * (size_t)pl->n_carrier : 0);
}

static int txf_workspace(ofdm_rx_plan* pl, int64_t ch, bool scr, bool sweep, TxfBuffers& b,
                         const TxfExtras& x = TxfExtras()) {
  const size_t cs = pl->f64 ? sizeof(c64) : sizeof(c32);
  const size_t fs = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t frame_bits = (size_t)pl->nd * pl->n_symb * pl->bps;
  const size_t t_bytes = a256(cs * fs * ch), p_bytes = a256(8 * (size_t)pl->n_symb * ch);
  const size_t b_bytes = scr ? a256(frame_bits * ch) : 0;
  const size_t r_bytes = sweep ? t_bytes : 0, f_bytes = sweep ? a256((size_t)pl->frame_words * 4 * ch) : 0;
  const size_t d_bytes = x.imp ? a256(8 * (size_t)ch) : 0;
  const size_t a_bytes = a256(sizeof(c64) * (size_t)x.fade_taps * ch);
  const size_t h_bytes = x.hest ? a256(cs * (size_t)pl->n_carrier * ch) : 0;
  const size_t need = t_bytes + p_bytes + 2 * b_bytes + r_bytes + f_bytes + 2 * d_bytes + a_bytes + h_bytes;
  if (pl->ws_txf_bytes < need) {
    OFDM_HIP(hipStreamSynchronize(ctx().stream));
    if (pl->ws_txf) { (void)hipFree(pl->ws_txf); pl->ws_txf = nullptr; pl->ws_txf_bytes = 0; }
    OFDM_HIP(hipMalloc(&pl->ws_txf, need));
    pl->ws_txf_bytes = need;
  }
  unsigned char* base = (unsigned char*)pl->ws_txf;
  b.tx = base;
  b.partial = (double*)(base + t_bytes);
  unsigned char* q = base + t_bytes + p_bytes;
  if (scr) { b.b0 = q; b.b1 = q + b_bytes; q += 2 * b_bytes; }
  if (sweep) { b.rx = q; b.ref = (uint32_t*)(q + r_bytes); q += r_bytes + f_bytes; }
  if (x.imp) { b.sto = (int64_t*)q; b.cfo = (double*)(q + d_bytes); q += 2 * d_bytes; }
  if (x.fade_taps) { b.amp = (c64*)q; q += a_bytes; }
  if (x.hest) b.hest = q;
  return OFDM_OK;
}

static int64_t txf_chunk(const ofdm_rx_plan* pl, bool scr, bool sweep, int64_t n_frames, int64_t user_cap,
                         const TxfExtras& x = TxfExtras()) {
  int64_t ch = user_cap > 0 ? user_cap : std::max<int64_t>(1, (int64_t)(TXF_WS_BUDGET / txf_frame_bytes(pl, scr, sweep, x)));
  return std::max<int64_t>(1, std::min<int64_t>({ch, n_frames, 65535}));
}

// one chunk of nf frames (streams stream0 ..): rx, the packed payload bits (ref) and the packed scrambled bits (scref)
// imp (optional): the Task-4 impairments, the channel pass of tx_channel_imp_kernel
// fade (optional): a channel per frame -- the draws into fade->amp (and fade->taps_out), the channel pass of
// tx_channel_fade_kernel; with imp too, both draws and the channel pass of tx_channel_imp_fade_kernel
static int txf_generate(ofdm_rx_plan* pl, const TxfChannel& ch, double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0,
                        int64_t nf, const uint8_t* scr_reg15, const TxfBuffers& b, void* rx, uint32_t* ref, uint32_t* scref,
                        const TxfImp* imp = nullptr, const TxfFade* fade = nullptr) {
  const int64_t frame_bits = (int64_t)pl->nd * pl->n_symb * pl->bps;
  OFDM_TRY(tx_bits_device(pl, ref, scr_reg15 ? b.b0 : nullptr, k0, k1, stream0, nf));
  if (scr_reg15) {                                              // Scrambler.m per frame, register reset (T5:58-69)
    OFDM_TRY(ofdm_Scrambler_frames(scr_reg15, b.b0, frame_bits, nf, b.b1, OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0)));
    if (scref) OFDM_TRY(tx_pack_bits_device(pl, b.b1, scref, nf));
  }
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &tw));
  const uint8_t* sc = scr_reg15 ? b.b1 : nullptr;
#define CALL(NN)                                                                                       \
  if (pl->f64) OFDM_TRY((launch_symbols<double, NN>(pl, tw, b.tx, b.partial, sc, k0, k1, stream0, nf))); \
  else OFDM_TRY((launch_symbols<float, NN>(pl, tw, b.tx, b.partial, sc, k0, k1, stream0, nf)));
  OFDM_FFT_DISPATCH(pl->nfft, CALL)
#undef CALL
  if (imp)
    OFDM_TRY(tx_draw_device(pl, imp->sto, imp->cfo, imp->sto_mode, imp->sto_value, imp->cfo_mode, imp->cfo_value, k0, k1,
                            stream0, nf));
  if (fade) {
    const int n_taps = (int)ch.delay.size();
    hipLaunchKernelGGL(tx_fade_draw_kernel, dim3(cdiv_u(nf * n_taps, 256)), dim3(256), 0, ctx().stream, fade->amp,
                       fade->taps_out, fade->gains, n_taps, k0, k1, stream0, nf);
    OFDM_TRY(check_launch("tx_fade_draw_kernel"));
  }
  if (pl->f64) OFDM_TRY(launch_channel<double>(pl, ch, b.tx, rx, b.partial, snr_lin, k0, k1, stream0, imp, fade, nf));
  else OFDM_TRY(launch_channel<float>(pl, ch, b.tx, rx, b.partial, snr_lin, k0, k1, stream0, imp, fade, nf));
  return OFDM_OK;
}

// bytes per frame of the ofdm_rx_chain_task4 arena (pl->ws_t4): t4_frame_bytes, beside t4_arena_layout in t4_route.hpp
static size_t t4_frame_bytes(const ofdm_rx_plan* pl) {
  return t4_frame_bytes(T4Shape{pl->nfft, pl->t_guard, pl->n_symb, pl->n_carrier, pl->np, pl->f64, 0, 0, 0, 0}, pl->frame_words);
}

static int txf_check_modes(int sto_mode, int cfo_mode, const char* what) {
  OFDM_ARG(sto_mode >= 0 && sto_mode <= 2 && cfo_mode >= 0 && cfo_mode <= 2, "%s: sto_mode / cfo_mode must be 0, 1 or 2", what);
  return OFDM_OK;
}

// the sweeps' Scrambler rule: with the Scrambler on the plan descrambles with the same register, else not at all
static int txf_check_descrambler(const ofdm_rx_plan* pl, const uint8_t* scr_reg15, const char* what) {
  if (scr_reg15) {                                              // errors against the payload: the plan must descramble
    uint32_t d = DESCR_ON;
    for (int m = 1; m <= 14; ++m) {
      OFDM_ARG(scr_reg15[m - 1] <= 1, "%s: register entries must be 0 or 1", what);
      d |= (uint32_t)scr_reg15[m - 1] << (m - 1);
    }
    OFDM_ARG(pl->descr == d, "%s: with the Scrambler on the plan needs a DeScrambler with the same register "
                             "(ofdm_rx_plan_set_descrambler)", what);
  } else {
    OFDM_ARG(!(pl->descr & DESCR_ON), "%s: the plan descrambles but the frames are not scrambled", what);
  }
  return OFDM_OK;
}

static int txf_check_plan(ofdm_rx_plan* pl, int flags, int64_t frame0, int64_t n_frames, const char* what) {
  OFDM_PLAN_DEVICE(pl);
  OFDM_ARG((is_f64(flags) ? 1 : 0) == pl->f64, "%s: precision flag differs from the plan's", what);
  OFDM_ARG(pl->nd >= 1, "%s: the plan has no data carriers", what);
  OFDM_ARG(pl->pilots_in_band, "%s: pilots outside 1..N_carrier are not supported", what);
  OFDM_ARG(fft_size_ok(pl->nfft) && pl->t_guard <= pl->nfft, "%s: unsupported Nfft %d / T_guard %d", what, pl->nfft,
           pl->t_guard);
  OFDM_ARG(frame0 >= 0 && n_frames >= 0 && frame0 + n_frames < ((int64_t)1 << 32),
           "%s: frame index outside the 32-bit stream range", what);
  return OFDM_OK;
}

// the body of the generator entries: n_frames frames from frame0 on in chunks of the plan-owned workspace.
// imp (optional): the Task-4 impairments -- the draws go to sto_out / cfo_out when they are given, else to the workspace
// fade (optional): a channel per frame on ch's delays -- the amplitudes go to the workspace and to taps_out when it is given
static int txf_frames(ofdm_rx_plan* pl, const TxfChannel& ch, double snr_db, uint64_t seed, int64_t frame0,
                      int64_t n_frames, const uint8_t* scr_reg15, const TxfImp* imp, const TxfFade* fade, void* rx_out,
                      uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out, int64_t* sto_out, double* cfo_out, double* taps_out,
                      int flags) {
  if (n_frames == 0) return OFDM_OK;
  OFDM_TRY(tx_dict_device(pl));
  const size_t cs = csize(flags);
  const int64_t frame_samples = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t fb = (size_t)pl->frame_words * 4;
  Stage st(flags);
  const int n_taps = fade ? (int)ch.delay.size() : 0;
  void *drx, *dref, *dscref, *dsto, *dcfo, *dtaps;
  OFDM_TRY(st.out(rx_out, cs * (size_t)frame_samples * n_frames, &drx));
  OFDM_TRY(st.out(ref_bits_out, fb * n_frames, &dref));
  OFDM_TRY(st.out(sc_ref_bits_out, fb * n_frames, &dscref));
  OFDM_TRY(st.out(sto_out, sizeof(int64_t) * (size_t)n_frames, &dsto));
  OFDM_TRY(st.out(cfo_out, sizeof(double) * (size_t)n_frames, &dcfo));
  OFDM_TRY(st.out(taps_out, sizeof(c64) * (size_t)n_taps * n_frames, &dtaps));
  const bool scr = scr_reg15 != nullptr;
  TxfExtras x;
  x.imp = imp != nullptr;
  x.fade_taps = n_taps;
  const int64_t CH = txf_chunk(pl, scr, false, n_frames, 0, x);
  TxfBuffers b;
  OFDM_TRY(txf_workspace(pl, CH, scr, false, b, x));
  const double snr_lin = std::pow(10.0, snr_db / 10.0);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  TxfImp ci;
  if (imp) ci = *imp;
  TxfFade cf;
  if (fade) cf = *fade;
  cf.amp = b.amp;
  for (int64_t c0 = 0; c0 < n_frames; c0 += CH) {
    const int64_t nf = std::min<int64_t>(CH, n_frames - c0);
    ci.sto = dsto ? (int64_t*)dsto + c0 : b.sto;
    ci.cfo = dcfo ? (double*)dcfo + c0 : b.cfo;
    cf.taps_out = dtaps ? (c64*)dtaps + c0 * n_taps : nullptr;
    OFDM_TRY(txf_generate(pl, ch, snr_lin, k0, k1, (uint32_t)(frame0 + c0), nf, scr_reg15, b,
                          (unsigned char*)drx + cs * (size_t)frame_samples * c0,
                          dref ? (uint32_t*)((uint8_t*)dref + fb * c0) : nullptr,
                          dscref ? (uint32_t*)((uint8_t*)dscref + fb * c0) : nullptr, imp ? &ci : nullptr,
                          fade ? &cf : nullptr));
  }
  return st.finish();
}

// the checks both sweeps make after their own argument checks
static int txf_check_sweep(ofdm_rx_plan* pl, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                           int64_t frames_per_point, int64_t frame0, int flags, const char* what) {
  OFDM_ARG(n_points == 0 || (snr_db && seeds), "%s: snr_db / seeds missing", what);
  OFDM_ARG(n_points < ((int64_t)1 << 31), "%s: too many points", what);
  return txf_check_plan(pl, flags, frame0, frames_per_point, what);
}

// the outputs both sweeps have: per point the bit errors and MER sums, per frame the errors and MER sums
struct TxfSweepOut {
  void *err = nullptr, *fe = nullptr, *mer = nullptr, *fm = nullptr;
};

// stages the common outputs; with no frames the per-point sums are zeroed, else the per-frame values of every point
// (reduced once after the last chunk) get scratch where the caller wants none
static int txf_sweep_outputs(Stage& st, int64_t n_points, int64_t frames_per_point, uint64_t* errors_out,
                             uint32_t* frame_errors_out, double* mer_sums_out, double* frame_mer_sums_out, TxfSweepOut& o) {
  const size_t np = (size_t)n_points, nf = (size_t)(n_points * frames_per_point);
  OFDM_TRY(st.out(errors_out, sizeof(uint64_t) * np, &o.err));
  OFDM_TRY(st.out(frame_errors_out, sizeof(uint32_t) * nf, &o.fe));
  OFDM_TRY(st.out(mer_sums_out, sizeof(double) * 2 * np, &o.mer));
  OFDM_TRY(st.out(frame_mer_sums_out, sizeof(double) * 2 * nf, &o.fm));
  if (frames_per_point == 0) {
    OFDM_HIP(hipMemsetAsync(o.err, 0, sizeof(uint64_t) * np, ctx().stream));
    if (o.mer) OFDM_HIP(hipMemsetAsync(o.mer, 0, sizeof(double) * 2 * np, ctx().stream));
    return OFDM_OK;
  }
  if (!o.fe) OFDM_TRY(st.scratch(sizeof(uint32_t) * nf, &o.fe));
  if (o.mer && !o.fm) OFDM_TRY(st.scratch(sizeof(double) * 2 * nf, &o.fm));
  return OFDM_OK;
}

// every point of a sweep, chunk by chunk of at most CH frames: the chunk generated into the workspace (imp: with the Task-4
// impairments, the draws of the sweep's frame k at imp->sto[k] / imp->cfo[k]; fade: with a channel per frame, the chunk's
// amplitudes at b.amp), then decode(b, nf, o) with o the sweep index of the chunk's first frame.  x: the workspace's extras.
template <typename Decode>
static int txf_sweep_points(ofdm_rx_plan* pl, const TxfChannel& ch, const double* snr_db, const uint64_t* seeds,
                            int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15, int64_t CH,
                            const TxfImp* imp, const TxfFade* fade, const TxfExtras& x, Decode&& decode) {
  OFDM_TRY(tx_dict_device(pl));
  TxfBuffers b;
  OFDM_TRY(txf_workspace(pl, CH, scr_reg15 != nullptr, true, b, x));
  TxfImp ci;
  if (imp) ci = *imp;
  TxfFade cf;
  if (fade) cf = *fade;
  cf.amp = b.amp;
  for (int64_t p = 0; p < n_points; ++p) {
    const double snr_lin = std::pow(10.0, snr_db[p] / 10.0);
    const uint32_t k0 = (uint32_t)seeds[p], k1 = (uint32_t)(seeds[p] >> 32);
    for (int64_t c0 = 0; c0 < frames_per_point; c0 += CH) {
      const int64_t nf = std::min<int64_t>(CH, frames_per_point - c0);
      const int64_t o = p * frames_per_point + c0;
      if (imp) { ci.sto = imp->sto + o; ci.cfo = imp->cfo + o; }
      OFDM_TRY(txf_generate(pl, ch, snr_lin, k0, k1, (uint32_t)(frame0 + c0), nf, scr_reg15, b, b.rx, b.ref, nullptr,
                            imp ? &ci : nullptr, fade ? &cf : nullptr));
      OFDM_TRY(decode(b, nf, o));
    }
  }
  return OFDM_OK;
}

// the per-point MER sums of a sweep with MER: the fixed-order reduction of the per-frame sums
static int txf_point_mer(const TxfSweepOut& o, int64_t n_points, int64_t frames_per_point) {
  if (!o.mer) return OFDM_OK;
  hipLaunchKernelGGL(t4_point_mer_kernel<2>, dim3((unsigned)n_points), dim3(256), 0, ctx().stream, (const double*)o.fm,
                     frames_per_point, (double*)o.mer);
  return check_launch("t4_point_mer_kernel");
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_tx_frames_fused(ofdm_rx_plan* pl, const void* h, int h_len, double snr_db, uint64_t seed, int64_t frame0,
                                    int64_t n_frames, const uint8_t* scr_reg15, void* rx_out, uint8_t* ref_bits_out,
                                    uint8_t* sc_ref_bits_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_frames >= 0 && rx_out, "tx_frames_fused: bad arguments");
  OFDM_TRY(txf_check_plan(pl, flags, frame0, n_frames, "tx_frames_fused"));
  OFDM_ARG(scr_reg15 || !sc_ref_bits_out, "tx_frames_fused: sc_ref_bits_out needs the Scrambler register");
  TxfChannel ch;
  OFDM_TRY(txf_channel(h, h_len, pl->f64 != 0, ch));
  return txf_frames(pl, ch, snr_db, seed, frame0, n_frames, scr_reg15, nullptr, nullptr, rx_out, ref_bits_out,
                    sc_ref_bits_out, nullptr, nullptr, nullptr, flags);
}

extern "C" int ofdm_tx_frames_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                     double snr_db, uint64_t seed, int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15,
                                     void* rx_out, uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out, double* taps_out,
                                     int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_frames >= 0 && rx_out, "tx_frames_fading: bad arguments");
  OFDM_TRY(txf_check_plan(pl, flags, frame0, n_frames, "tx_frames_fading"));
  OFDM_ARG(scr_reg15 || !sc_ref_bits_out, "tx_frames_fading: sc_ref_bits_out needs the Scrambler register");
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_fading(tap_delay, tap_power, n_taps, "tx_frames_fading", ch, fade));
  return txf_frames(pl, ch, snr_db, seed, frame0, n_frames, scr_reg15, nullptr, &fade, rx_out, ref_bits_out, sc_ref_bits_out,
                    nullptr, nullptr, taps_out, flags);
}

extern "C" int ofdm_tx_frames_fused_ex(ofdm_rx_plan* pl, const void* h, int h_len, double snr_db, uint64_t seed,
                                       int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, int sto_mode,
                                       int64_t sto_value, int cfo_mode, double cfo_value, void* rx_out, uint8_t* ref_bits_out,
                                       uint8_t* sc_ref_bits_out, int64_t* sto_out, double* cfo_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_frames >= 0 && rx_out, "tx_frames_fused_ex: bad arguments");
  OFDM_TRY(txf_check_plan(pl, flags, frame0, n_frames, "tx_frames_fused_ex"));
  OFDM_TRY(txf_check_modes(sto_mode, cfo_mode, "tx_frames_fused_ex"));
  OFDM_ARG(scr_reg15 || !sc_ref_bits_out, "tx_frames_fused_ex: sc_ref_bits_out needs the Scrambler register");
  TxfImp imp;
  imp.sto_mode = sto_mode; imp.sto_value = sto_value; imp.cfo_mode = cfo_mode; imp.cfo_value = cfo_value;
  TxfChannel ch;
  OFDM_TRY(txf_channel(h, h_len, pl->f64 != 0, ch));
  return txf_frames(pl, ch, snr_db, seed, frame0, n_frames, scr_reg15, &imp, nullptr, rx_out, ref_bits_out, sc_ref_bits_out,
                    sto_out, cfo_out, nullptr, flags);
}

extern "C" int ofdm_tx_frames_fading_ex(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                        double snr_db, uint64_t seed, int64_t frame0, int64_t n_frames,
                                        const uint8_t* scr_reg15, int sto_mode, int64_t sto_value, int cfo_mode,
                                        double cfo_value, void* rx_out, uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out,
                                        double* taps_out, int64_t* sto_out, double* cfo_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_frames >= 0 && rx_out, "tx_frames_fading_ex: bad arguments");
  OFDM_TRY(txf_check_plan(pl, flags, frame0, n_frames, "tx_frames_fading_ex"));
  OFDM_TRY(txf_check_modes(sto_mode, cfo_mode, "tx_frames_fading_ex"));
  OFDM_ARG(scr_reg15 || !sc_ref_bits_out, "tx_frames_fading_ex: sc_ref_bits_out needs the Scrambler register");
  TxfImp imp;
  imp.sto_mode = sto_mode; imp.sto_value = sto_value; imp.cfo_mode = cfo_mode; imp.cfo_value = cfo_value;
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_fading(tap_delay, tap_power, n_taps, "tx_frames_fading_ex", ch, fade));
  return txf_frames(pl, ch, snr_db, seed, frame0, n_frames, scr_reg15, &imp, &fade, rx_out, ref_bits_out, sc_ref_bits_out,
                    sto_out, cfo_out, taps_out, flags);
}

// the body of both Task-5 sweep entries, after their argument checks: ch the static channel, or with fade the delay line of a
// channel per frame; nmse_sums_out / frame_nmse_out (fading only): the channel-estimate error sums
static int t5_sweep(ofdm_rx_plan* pl, const TxfChannel& ch, const TxfFade* fade, const double* snr_db, const uint64_t* seeds,
                    int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                    int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out, double* mer_sums_out,
                    double* frame_mer_sums_out, double* nmse_sums_out, double* frame_nmse_out, int flags) {
  if (n_points == 0) return OFDM_OK;
  Stage st(flags);
  TxfSweepOut o;
  OFDM_TRY(txf_sweep_outputs(st, n_points, frames_per_point, errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out,
                             o));
  void *dns, *dfn;
  OFDM_TRY(st.out(nmse_sums_out, sizeof(double) * (size_t)n_points, &dns));
  OFDM_TRY(st.out(frame_nmse_out, sizeof(double) * (size_t)(n_points * frames_per_point), &dfn));
  if (frames_per_point == 0) {
    if (dns) OFDM_HIP(hipMemsetAsync(dns, 0, sizeof(double) * (size_t)n_points, ctx().stream));
    return st.finish();
  }
  if (dns && !dfn) OFDM_TRY(st.scratch(sizeof(double) * (size_t)(n_points * frames_per_point), &dfn));
  TxfExtras x;
  x.fade_taps = fade ? (int)ch.delay.size() : 0;
  x.hest = dfn != nullptr;
  const int64_t CH = txf_chunk(pl, scr_reg15 != nullptr, true, frames_per_point, max_frames_per_chunk, x);
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  TxfDelays dl{};
  dl.n = x.fade_taps;
  for (int t = 0; t < dl.n; ++t) dl.d[t] = ch.delay[t];
  // a plan in the h = ifft(H_LS) MMSE mode estimates every point at the point's own SNR (a host scalar of the stage's launch)
  OFDM_TRY(txf_sweep_points(pl, ch, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, CH, nullptr, fade, x,
                            [&](const TxfBuffers& b, int64_t nf, int64_t k) {
                              const double inv_snr = 1.0 / std::pow(10.0, snr_db[k / frames_per_point] * 0.1);
                              OFDM_TRY(rx_chain_task5_run(pl, b.rx, nf, nullptr, (const uint8_t*)b.ref,
                                                          (uint32_t*)o.fe + k, b.hest, nullptr,
                                                          o.fm ? (double*)o.fm + 2 * k : nullptr, rxflags, inv_snr));
                              if (!dfn) return (int)OFDM_OK;
                              if (pl->f64)
                                hipLaunchKernelGGL(t5_frame_nmse_kernel<double>, dim3((unsigned)nf), dim3(256), 0, ctx().stream,
                                                   (const c64*)b.amp, (const c64*)b.hest, dl, (int64_t)dl.n, pl->nfft,
                                                   pl->n_carrier, (double*)dfn + k);
                              else
                                hipLaunchKernelGGL(t5_frame_nmse_kernel<float>, dim3((unsigned)nf), dim3(256), 0, ctx().stream,
                                                   (const c64*)b.amp, (const c32*)b.hest, dl, (int64_t)dl.n, pl->nfft,
                                                   pl->n_carrier, (double*)dfn + k);
                              return check_launch("t5_frame_nmse_kernel");
                            }));
  hipLaunchKernelGGL(ber_point_reduce_kernel, dim3((unsigned)n_points), dim3(256), 0, ctx().stream, (const uint32_t*)o.fe,
                     frames_per_point, (unsigned long long*)o.err);
  OFDM_TRY(check_launch("ber_point_reduce_kernel"));
  OFDM_TRY(txf_point_mer(o, n_points, frames_per_point));
  if (dns) {
    hipLaunchKernelGGL(t4_point_mer_kernel<1>, dim3((unsigned)n_points), dim3(256), 0, ctx().stream, (const double*)dfn,
                       frames_per_point, (double*)dns);
    OFDM_TRY(check_launch("t4_point_mer_kernel"));
  }
  return st.finish();
}

extern "C" int ofdm_ber_sweep_task5_ex(ofdm_rx_plan* pl, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                                       int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                       int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                                       double* mer_sums_out, double* frame_mer_sums_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_points >= 0 && frames_per_point >= 0 && max_frames_per_chunk >= 0 && errors_out,
           "ber_sweep_task5: bad arguments");
  OFDM_TRY(txf_check_sweep(pl, snr_db, seeds, n_points, frames_per_point, frame0, flags, "ber_sweep_task5"));
  OFDM_ARG(!pl->d_wt || n_points <= 1, "ber_sweep_task5: an MMSE-mode plan is built for one SNR (n_points must be 1)");
  OFDM_TRY(txf_check_descrambler(pl, scr_reg15, "ber_sweep_task5"));
  TxfChannel ch;
  OFDM_TRY(txf_channel(h, h_len, pl->f64 != 0, ch));
  return t5_sweep(pl, ch, nullptr, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk,
                  errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nullptr, nullptr, flags);
}

extern "C" int ofdm_ber_sweep_task5_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                           const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                           int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                           int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                                           double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                           double* frame_nmse_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_points >= 0 && frames_per_point >= 0 && max_frames_per_chunk >= 0 && errors_out,
           "ber_sweep_task5_fading: bad arguments");
  OFDM_TRY(txf_check_sweep(pl, snr_db, seeds, n_points, frames_per_point, frame0, flags, "ber_sweep_task5_fading"));
  OFDM_ARG(!pl->d_wt, "ber_sweep_task5_fading: an MMSE-mode plan is built for one channel h (ofdm_rx_plan_set_mmse)");
  OFDM_TRY(txf_check_descrambler(pl, scr_reg15, "ber_sweep_task5_fading"));
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_fading(tap_delay, tap_power, n_taps, "ber_sweep_task5_fading", ch, fade));
  return t5_sweep(pl, ch, &fade, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk,
                  errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out, flags);
}

extern "C" int ofdm_ber_sweep_task5(ofdm_rx_plan* pl, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                                    int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                    int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out, int flags) {
  return ofdm_ber_sweep_task5_ex(pl, h, h_len, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15,
                                 max_frames_per_chunk, errors_out, frame_errors_out, nullptr, nullptr, flags);
}

// the body of the Task-4 sweep entries: the argument checks they share, then ch the static channel, or with fade the delay line
// of a channel per frame; nmse_sums_out / frame_nmse_out (optional): the channel-estimate error sums against ch's H (static:
// one H for every frame) or the frame's own H_f (fade)
static int t4_sweep(ofdm_rx_plan* pl, const TxfChannel& ch, const TxfFade* fade, int sto_mode, int64_t sto_value, int cfo_mode,
                    double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                    const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                    const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* status_counts_out,
                    double* cfo_abs_err_out, uint32_t* frame_errors_out, int64_t mer_skip, double* mer_sums_out,
                    double* frame_mer_sums_out, double* nmse_sums_out, double* frame_nmse_out, int flags) {
  OFDM_ARG(max_frames_per_chunk >= 0 && max_frames_per_chunk <= 65535,
           "ber_sweep_task4: max_frames_per_chunk must be 0..65535 (the limit of rx_chain_task4)");
  OFDM_TRY(txf_check_sweep(pl, snr_db, seeds, n_points, frames_per_point, frame0, flags, "ber_sweep_task4"));
  OFDM_TRY(txf_check_modes(sto_mode, cfo_mode, "ber_sweep_task4"));
  OFDM_TRY(txf_check_descrambler(pl, scr_reg15, "ber_sweep_task4"));
  OFDM_ARG(mer_skip >= 0 && mer_skip < (int64_t)pl->nd * pl->n_symb,
           "ber_sweep_task4_ex: mer_skip must be 0 .. nd * N_symb - 1 (%lld)", (long long)mer_skip);
  OFDM_ARG(!(nmse_sums_out || frame_nmse_out) || mp_desync,
           "ber_sweep_task4: the NMSE outputs need mp_desync (without estimate_channel there is no estimate)");
  if (n_points == 0) return OFDM_OK;
  Stage st(flags);
  const int64_t NF = n_points * frames_per_point;
  TxfSweepOut o;
  OFDM_TRY(txf_sweep_outputs(st, n_points, frames_per_point, errors_out, frame_errors_out, mer_sums_out, frame_mer_sums_out,
                             o));
  void *dsc, *dabs, *dns, *dfn;
  OFDM_TRY(st.out(status_counts_out, sizeof(uint64_t) * 4 * (size_t)n_points, &dsc));
  OFDM_TRY(st.out(cfo_abs_err_out, sizeof(double) * (size_t)n_points, &dabs));
  OFDM_TRY(st.out(nmse_sums_out, sizeof(double) * (size_t)n_points, &dns));
  OFDM_TRY(st.out(frame_nmse_out, sizeof(double) * (size_t)NF, &dfn));
  hipStream_t s = ctx().stream;
  if (frames_per_point == 0) {
    if (dsc) OFDM_HIP(hipMemsetAsync(dsc, 0, sizeof(uint64_t) * 4 * (size_t)n_points, s));
    if (dabs) OFDM_HIP(hipMemsetAsync(dabs, 0, sizeof(double) * (size_t)n_points, s));
    if (dns) OFDM_HIP(hipMemsetAsync(dns, 0, sizeof(double) * (size_t)n_points, s));
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
  if (dns && !dfn) OFDM_TRY(st.scratch(sizeof(double) * (size_t)NF, &dfn));
  const bool scr = scr_reg15 != nullptr;
  const int n_taps = (int)ch.delay.size();
  TxfExtras x;
  x.imp = true;
  x.fade_taps = fade ? n_taps : 0;
  x.hest = dfn != nullptr;
  // default chunk: the generator workspace and the Task-4 arena (shared with ofdm_task5_part2_tile) budgeted together
  int64_t CH = max_frames_per_chunk;
  if (CH == 0)                                                  // (+ the per-frame MER sums when they are wanted)
    CH = std::max<int64_t>(1, (int64_t)(2 * TXF_WS_BUDGET /
                                        (txf_frame_bytes(pl, scr, true, x) + t4_frame_bytes(pl) + (o.fm ? 16 : 0))));
  CH = std::max<int64_t>(1, std::min<int64_t>({CH, frames_per_point, 65535}));
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  TxfImp imp;
  imp.sto_mode = sto_mode; imp.sto_value = sto_value; imp.cfo_mode = cfo_mode; imp.cfo_value = cfo_value;
  imp.sto = (int64_t*)dsto;
  imp.cfo = (double*)dcfo;
  TxfDelays dl{};
  void* dstatic = nullptr;                                      // NMSE against a static channel: its taps, read with stride 0
  if (dfn) {
    dl.n = n_taps;
    for (int t = 0; t < n_taps; ++t) dl.d[t] = ch.delay[t];
    if (!fade) {
      TxfAmps sa{};
      for (int t = 0; t < n_taps; ++t) sa.a[t] = ch.amp[t];
      OFDM_TRY(st.scratch(sizeof(c64) * (size_t)std::max(n_taps, 1), &dstatic));   // an all-zero h has no taps: H = 0
      hipLaunchKernelGGL(tx_static_amp_kernel, dim3(1), dim3(64), 0, s, (c64*)dstatic, sa, n_taps);
      OFDM_TRY(check_launch("tx_static_amp_kernel"));
    }
  }
  OFDM_TRY(txf_sweep_points(pl, ch, snr_db, seeds, n_points, frames_per_point, frame0, scr_reg15, CH, &imp, fade, x,
                            [&](const TxfBuffers& b, int64_t nf, int64_t k) {
                              OFDM_TRY(ofdm_rx_chain_task4_ex(pl, b.rx, nf, time_desync, freq_desync, mp_desync, nullptr,
                                                              (const uint8_t*)b.ref, (uint32_t*)o.fe + k, (int64_t*)dtg + k,
                                                              (double*)dfo + k, (int32_t*)difo + k, (int32_t*)dstat + k,
                                                              b.hest, mer_skip, o.fm ? (double*)o.fm + 2 * k : nullptr,
                                                              rxflags));
                              if (!dfn) return (int)OFDM_OK;
                              const c64* amp = fade ? (const c64*)b.amp : (const c64*)dstatic;
                              const int64_t stride = fade ? n_taps : 0;
                              if (pl->f64)
                                hipLaunchKernelGGL(t5_frame_nmse_kernel<double>, dim3((unsigned)nf), dim3(256), 0, s, amp,
                                                   (const c64*)b.hest, dl, stride, pl->nfft, pl->n_carrier, (double*)dfn + k);
                              else
                                hipLaunchKernelGGL(t5_frame_nmse_kernel<float>, dim3((unsigned)nf), dim3(256), 0, s, amp,
                                                   (const c32*)b.hest, dl, stride, pl->nfft, pl->n_carrier, (double*)dfn + k);
                              return check_launch("t5_frame_nmse_kernel");
                            }));
  hipLaunchKernelGGL(t4_point_reduce_kernel, dim3((unsigned)n_points), dim3(256), 0, s, (const uint32_t*)o.fe,
                     (const int32_t*)dstat, (const double*)dfo, (const int32_t*)difo, (const double*)dcfo, frames_per_point,
                     freq_desync ? 1 : 0, (unsigned long long*)o.err, (unsigned long long*)dsc, (double*)dabs);
  OFDM_TRY(check_launch("t4_point_reduce_kernel"));
  OFDM_TRY(txf_point_mer(o, n_points, frames_per_point));
  if (dns) {
    hipLaunchKernelGGL(t4_point_mer_kernel<1>, dim3((unsigned)n_points), dim3(256), 0, s, (const double*)dfn,
                       frames_per_point, (double*)dns);
    OFDM_TRY(check_launch("t4_point_mer_kernel"));
  }
  return st.finish();
}

extern "C" int ofdm_ber_sweep_task4_nmse(ofdm_rx_plan* pl, const void* h, int h_len, int sto_mode, int64_t sto_value,
                                         int cfo_mode, double cfo_value, int time_desync, int freq_desync, int mp_desync,
                                         const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                         int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                         int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* status_counts_out,
                                         double* cfo_abs_err_out, uint32_t* frame_errors_out, int64_t mer_skip,
                                         double* mer_sums_out, double* frame_mer_sums_out, double* nmse_sums_out,
                                         double* frame_nmse_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_points >= 0 && frames_per_point >= 0 && errors_out, "ber_sweep_task4: bad arguments");
  TxfChannel ch;
  OFDM_TRY(txf_channel(h, h_len, is_f64(flags), ch));
  return t4_sweep(pl, ch, nullptr, sto_mode, sto_value, cfo_mode, cfo_value, time_desync, freq_desync, mp_desync, snr_db, seeds,
                  n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk, errors_out, status_counts_out,
                  cfo_abs_err_out, frame_errors_out, mer_skip, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out,
                  flags);
}

extern "C" int ofdm_ber_sweep_task4_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                           int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                                           int freq_desync, int mp_desync, const double* snr_db, const uint64_t* seeds,
                                           int64_t n_points, int64_t frames_per_point, int64_t frame0,
                                           const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                                           uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                                           int64_t mer_skip, double* mer_sums_out, double* frame_mer_sums_out,
                                           double* nmse_sums_out, double* frame_nmse_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && n_points >= 0 && frames_per_point >= 0 && errors_out, "ber_sweep_task4_fading: bad arguments");
  TxfChannel ch;
  TxfFade fade;
  OFDM_TRY(txf_fading(tap_delay, tap_power, n_taps, "ber_sweep_task4_fading", ch, fade));
  return t4_sweep(pl, ch, &fade, sto_mode, sto_value, cfo_mode, cfo_value, time_desync, freq_desync, mp_desync, snr_db, seeds,
                  n_points, frames_per_point, frame0, scr_reg15, max_frames_per_chunk, errors_out, status_counts_out,
                  cfo_abs_err_out, frame_errors_out, mer_skip, mer_sums_out, frame_mer_sums_out, nmse_sums_out, frame_nmse_out,
                  flags);
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
