// ofdm_tx_frames_fused: the reference-order frame generator in three sample passes (T5/Task5_part2.m:134,:148-152); the
// device-resident BER(SNR) sweeps on top of it are ofdm_ber_sweep.hip's.
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
// TX samples: one write, one read (+ halo), RX: one write -- 3 sample passes against ~9 for ofdm_tx_frames_ex's stages.
//
// ofdm_tx_frames_fused_ex adds the Task-4 impairments (T4/Main_model_Task_4.m:99-110, add_STO.m,
// add_CFO.m) in the reference order Noise -> add_STO -> add_CFO -> conv, still in three sample passes:
//   tx_channel_imp_kernel<T>        tx_channel_fused_kernel's body (tx_channel_body) with IMP on: its LDS load stage builds
//                                   z[m] = w[m + sto_f] e^{2 pi i cfo_f m / Nfft} for the segment and its halo, the noise of w
//                                   drawn at the SOURCE index m + sto_f (Noise comes before the shift).  The shift is uniform
//                                   per frame: no extra halo, the loads stay coalesced.
// The per-frame draws are tx_draw_kernel's (ofdm_txgen.hip), the draws of ofdm_tx_frames_ex.
//
// ofdm_tx_frames_fading draws a channel per frame (the Monte-Carlo realisations of T5/Task5_part2.m:148-155) on one tap-delay
// line, still in three sample passes:
//   tx_fade_draw_kernel             tap t of frame f: a = g_t e^{2 pi i u}, u from Philox counter (t, 0, frame0 + f, 3), double
//   tx_channel_fade_kernel<T>       tx_channel_body with FADE on: the delays and the halo stay in the kernel arguments (uniform
//                                   over the launch), the amplitudes of frame blockIdx.y are read once per workgroup into the
//                                   tail of the dynamic LDS, cast to T as the static path casts h
//
// ofdm_tx_frames_fading_ex puts both together for the Task-4 receiver (T4/Main_model_Task_4.m:94-110,:257-267 over the
// realisations of T5/Task5_part2.m:148-155):
//   tx_channel_imp_fade_kernel<T>   tx_channel_body with IMP and FADE on: the load stage is tx_channel_imp_kernel's (Noise ->
//                                   add_STO -> add_CFO), the frame's amplitudes staged behind the segment as in
//                                   tx_channel_fade_kernel; the two per-frame draws stay independent (counter word 3 = 2 / 3)
//
// Host side: what a call decides -- its channel, the workspace regions and the chunk, the argument checks in the entry's
// order, the kernel, LDS and grid of the channel pass -- is txf_plan.hpp's, plain C++ tested without a GPU.  The four entries
// fill a TxfCall and a TxfGenOut and forward to one body (txf_frames): given impairments it launches the draw kernel and
// tx_channel_imp_kernel, else tx_channel_fused_kernel; given a TxfFade, tx_fade_draw_kernel and tx_channel_fade_kernel
// (tx_channel_imp_fade_kernel given impairments too).  The sweeps use txf_workspace and txf_generate (txf_generate.hpp).
//
// ofdm_tx_frames_payload is ofdm_tx_frames_fused_ex / _fading_ex with the caller's bits in place of the payload draw: the bit stage
// of a chunk is payload_frames_kernel (ofdm_payload.hip) instead of tx_bits_kernel, the symbol stage reads the bytes it wrote (or
// the Scrambler's), every other stage and every other draw is the same.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "fft_core.hpp"
#include "payload_plan.hpp"
#include "tx_philox.hpp"
#include "txf_generate.hpp"

namespace ofdm {
int tx_bits_device(const ofdm_rx_plan* pl, uint32_t* packed, uint8_t* bits, uint32_t k0, uint32_t k1, uint32_t stream0,
                   int64_t nf);
int tx_pack_bits_device(const ofdm_rx_plan* pl, const uint8_t* bits, uint32_t* packed, int64_t nf);
int tx_draw_device(const ofdm_rx_plan* pl, int64_t* sto, double* cfo, int sto_mode, int64_t sto_value, int cfo_mode,
                   double cfo_value, uint32_t k0, uint32_t k1, uint32_t stream0, int64_t nf);

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

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
TxfShape txf_shape(const ofdm_rx_plan* pl) {
  return TxfShape{pl->nfft, pl->t_guard, pl->n_symb, pl->n_carrier, pl->np, pl->nd, pl->bps, pl->frame_words, pl->f64,
                  pl->pilots_in_band, pl->descr, pl->d_wt != nullptr, pl->device, ctx().device};
}

int txf_refused(int id, const TxfWhy& w) {
  if (id == TXF_OK) return OFDM_OK;
  set_error("%s", w.text);
  return id == TXF_REFUSE_DEVICE ? OFDM_ERR_STATE : OFDM_ERR_ARG;
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

// the symbol stage of a chunk of nf frames: tx_symbols_fused_kernel in the plan's precision and Nfft (sc_bits: the frames' bits,
// one byte each, in place of the Philox payload; null: the payload draw)
int txf_symbols(const ofdm_rx_plan* pl, void* tx, double* partial, const uint8_t* sc_bits, uint32_t k0, uint32_t k1,
                uint32_t stream0, int64_t nf) {
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &tw));
#define CALL(NN)                                                                                       \
  if (pl->f64) OFDM_TRY((launch_symbols<double, NN>(pl, tw, tx, partial, sc_bits, k0, k1, stream0, nf))); \
  else OFDM_TRY((launch_symbols<float, NN>(pl, tw, tx, partial, sc_bits, k0, k1, stream0, nf)));
  OFDM_FFT_DISPATCH(pl->nfft, CALL)
#undef CALL
  return OFDM_OK;
}

// the channel pass txf_channel_pass chose: with imp the chunk's draws imp->sto / imp->cfo, with fade its amplitudes fade->amp
template <typename T>
static int launch_channel(const ofdm_rx_plan* pl, const TxfChannel& ch, const void* tx, void* rx, const double* partial,
                          double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0, const TxfImp* imp, const TxfFade* fade,
                          int64_t nf) {
  const TxfPass p = txf_channel_pass(txf_shape(pl), ch, imp != nullptr, fade != nullptr, nf);
  const dim3 grid(p.grid_x, p.grid_y);
  const void* const kernels[] = {(const void*)tx_channel_fused_kernel<T>, (const void*)tx_channel_imp_kernel<T>,
                                 (const void*)tx_channel_fade_kernel<T>, (const void*)tx_channel_imp_fade_kernel<T>};
  // > 64 KB for long channels: the attribute is per device, so it is set on every launch (not cached per process)
  OFDM_HIP(hipFuncSetAttribute(kernels[p.kernel], hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
  const double inv_nfft = 1.0 / (double)pl->nfft;
  switch (p.kernel) {
    case TXF_PASS_IMP_FADE:
      hipLaunchKernelGGL(tx_channel_imp_fade_kernel<T>, grid, dim3(256), p.lds, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx,
                         partial, pl->n_symb, p.len, snr_lin, k0, k1, stream0, imp->sto, imp->cfo, inv_nfft,
                         (const c64*)fade->amp, txf_taps<T>(ch));
      break;
    case TXF_PASS_FADE:
      hipLaunchKernelGGL(tx_channel_fade_kernel<T>, grid, dim3(256), p.lds, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                         pl->n_symb, p.len, snr_lin, k0, k1, stream0, (const c64*)fade->amp, txf_taps<T>(ch));
      break;
    case TXF_PASS_IMP:
      hipLaunchKernelGGL(tx_channel_imp_kernel<T>, grid, dim3(256), p.lds, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                         pl->n_symb, p.len, snr_lin, k0, k1, stream0, imp->sto, imp->cfo, inv_nfft, txf_taps<T>(ch));
      break;
    default:
      hipLaunchKernelGGL(tx_channel_fused_kernel<T>, grid, dim3(256), p.lds, ctx().stream, (const cx<T>*)tx, (cx<T>*)rx, partial,
                         pl->n_symb, p.len, snr_lin, k0, k1, stream0, txf_taps<T>(ch));
  }
  return check_launch(p.name);
}

int txf_workspace(ofdm_rx_plan* pl, int64_t ch, const TxfUse& u, TxfBuffers& b) {
  const TxfLayout l = txf_layout(txf_shape(pl), u, ch);
  if (pl->ws_txf_bytes < l.total) {
    OFDM_HIP(hipStreamSynchronize(ctx().stream));
    if (pl->ws_txf) { (void)hipFree(pl->ws_txf); pl->ws_txf = nullptr; pl->ws_txf_bytes = 0; }
    OFDM_HIP(hipMalloc(&pl->ws_txf, l.total));
    pl->ws_txf_bytes = l.total;
  }
  unsigned char* base = (unsigned char*)pl->ws_txf;
  auto at = [&](int r) { return l.bytes[r] ? base + l.off[r] : nullptr; };
  b.tx = at(TXF_R_TX);
  b.partial = (double*)at(TXF_R_PARTIAL);
  b.b0 = at(TXF_R_B0);
  b.b1 = at(TXF_R_B1);
  b.rx = at(TXF_R_RX);
  b.ref = (uint32_t*)at(TXF_R_REF);
  b.sto = (int64_t*)at(TXF_R_STO);
  b.cfo = (double*)at(TXF_R_CFO);
  b.amp = (c64*)at(TXF_R_AMP);
  b.hest = at(TXF_R_HEST);
  return OFDM_OK;
}

int txf_generate(ofdm_rx_plan* pl, const TxfChannel& ch, double snr_lin, uint32_t k0, uint32_t k1, uint32_t stream0, int64_t nf,
                 const uint8_t* scr_reg15, const TxfBuffers& b, void* rx, uint32_t* ref, uint32_t* scref, const TxfImp* imp,
                 const TxfFade* fade, const TxfPayload* src) {
  const int64_t frame_bits = (int64_t)pl->nd * pl->n_symb * pl->bps;
  if (src) OFDM_TRY(payload_frames_device(pl, *src, nf, b.b0, ref));   // the caller's bits: the only stage that differs
  else OFDM_TRY(tx_bits_device(pl, ref, scr_reg15 ? b.b0 : nullptr, k0, k1, stream0, nf));
  if (scr_reg15) {                                              // Scrambler.m per frame, register reset (T5:58-69)
    OFDM_TRY(ofdm_Scrambler_frames(scr_reg15, b.b0, frame_bits, nf, b.b1, OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0)));
    if (scref) OFDM_TRY(tx_pack_bits_device(pl, b.b1, scref, nf));
  }
  OFDM_TRY(txf_symbols(pl, b.tx, b.partial, scr_reg15 ? b.b1 : src ? b.b0 : nullptr, k0, k1, stream0, nf));
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

// where a generator call wants its frames: rx is mandatory, the others optional (sto / cfo: the draws of a call with
// impairments, else they go to the workspace; taps: the amplitudes of a fading call, [n_frames][n_taps] complex double)
struct TxfGenOut {
  void* rx;
  uint8_t *ref_bits, *sc_ref_bits;
  int64_t* sto;
  double* cfo;
  double* taps;
};

// the caller's payload of ofdm_tx_frames_payload, where `flags` says: frame f of the call carries the stream bits
// (first_frame + f) frame_bits .. (payload_plan.hpp)
struct TxfGivenBits {
  const uint8_t* payload;
  int64_t n_bits, first_frame;
  bool both_channels;                                // h and a tap-delay line are given: refused
};

// the body of the five generator entries: the checks of txf_generator_prelude (given: behind the payload's own,
// payload_generator_prelude), then c.n_frames frames from c.frame0 on in chunks of the plan-owned workspace.  imp: the entry's
// impairments (null: none, no draw kernel, the plain channel pass).  given: the bits in place of the payload draw.
static int txf_frames(ofdm_rx_plan* pl, TxfCall c, double snr_db, uint64_t seed, const TxfImp* imp, const TxfGenOut& out,
                      int flags, const TxfGivenBits* given = nullptr) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  c.plan = pl ? &s : nullptr;
  c.out = out.rx != nullptr;
  c.f64_flag = is_f64(flags);
  c.sc_ref_out = out.sc_ref_bits != nullptr;
  TxfChannel ch;
  TxfFade cf;
  TxfWhy why;
  if (given)
    OFDM_TRY(txf_refused(payload_generator_prelude(c, given->payload != nullptr, given->n_bits, given->first_frame,
                                                   given->both_channels, ch, cf.gains, why), why));
  else OFDM_TRY(txf_refused(txf_generator_prelude(c, ch, cf.gains, why), why));
  const int64_t n_frames = c.n_frames;
  if (n_frames == 0) return OFDM_OK;
  OFDM_TRY(tx_dict_device(pl));
  const size_t cs = csize(flags);
  const int64_t frame_samples = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t fb = (size_t)pl->frame_words * 4;
  Stage st(flags);
  const int n_taps = c.fading ? (int)ch.delay.size() : 0;
  void *drx, *dref, *dscref, *dsto, *dcfo, *dtaps;
  OFDM_TRY(st.out(out.rx, cs * (size_t)frame_samples * n_frames, &drx));
  OFDM_TRY(st.out(out.ref_bits, fb * n_frames, &dref));
  OFDM_TRY(st.out(out.sc_ref_bits, fb * n_frames, &dscref));
  OFDM_TRY(st.out(out.sto, sizeof(int64_t) * (size_t)n_frames, &dsto));
  OFDM_TRY(st.out(out.cfo, sizeof(double) * (size_t)n_frames, &dcfo));
  OFDM_TRY(st.out(out.taps, sizeof(c64) * (size_t)n_taps * n_frames, &dtaps));
  TxfUse u;
  u.scr = c.scr_reg15 != nullptr;
  u.imp = imp != nullptr;
  u.fade_taps = n_taps;
  u.payload = given != nullptr;
  TxfPayload src;
  if (given) {
    OFDM_TRY(payload_stage(st, given->payload, given->n_bits, &src.words));
    src.n_bits = given->n_bits;
    src.first_frame = given->first_frame;
  }
  const int64_t CH = txf_chunk(s, u, n_frames, 0);
  TxfBuffers b;
  OFDM_TRY(txf_workspace(pl, CH, u, b));
  const double snr_lin = std::pow(10.0, snr_db / 10.0);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  TxfImp ci;
  if (imp) ci = *imp;
  cf.amp = b.amp;
  for (int64_t c0 = 0; c0 < n_frames; c0 += CH) {
    const int64_t nf = std::min<int64_t>(CH, n_frames - c0);
    ci.sto = dsto ? (int64_t*)dsto + c0 : b.sto;
    ci.cfo = dcfo ? (double*)dcfo + c0 : b.cfo;
    cf.taps_out = dtaps ? (c64*)dtaps + c0 * n_taps : nullptr;
    src.frame = c0;
    OFDM_TRY(txf_generate(pl, ch, snr_lin, k0, k1, (uint32_t)(c.frame0 + c0), nf, c.scr_reg15, b,
                          (unsigned char*)drx + cs * (size_t)frame_samples * c0,
                          dref ? (uint32_t*)((uint8_t*)dref + fb * c0) : nullptr,
                          dscref ? (uint32_t*)((uint8_t*)dscref + fb * c0) : nullptr, imp ? &ci : nullptr,
                          c.fading ? &cf : nullptr, given ? &src : nullptr));
  }
  return st.finish();
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_tx_frames_fused(ofdm_rx_plan* pl, const void* h, int h_len, double snr_db, uint64_t seed, int64_t frame0,
                                    int64_t n_frames, const uint8_t* scr_reg15, void* rx_out, uint8_t* ref_bits_out,
                                    uint8_t* sc_ref_bits_out, int flags) {
  return txf_frames(pl, TxfCall("tx_frames_fused", frame0, n_frames, scr_reg15).with_h(h, h_len), snr_db, seed, nullptr,
                    TxfGenOut{rx_out, ref_bits_out, sc_ref_bits_out, nullptr, nullptr, nullptr}, flags);
}

extern "C" int ofdm_tx_frames_fading(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                     double snr_db, uint64_t seed, int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15,
                                     void* rx_out, uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out, double* taps_out,
                                     int flags) {
  return txf_frames(pl, TxfCall("tx_frames_fading", frame0, n_frames, scr_reg15).with_fading(tap_delay, tap_power, n_taps),
                    snr_db, seed, nullptr, TxfGenOut{rx_out, ref_bits_out, sc_ref_bits_out, nullptr, nullptr, taps_out}, flags);
}

extern "C" int ofdm_tx_frames_fused_ex(ofdm_rx_plan* pl, const void* h, int h_len, double snr_db, uint64_t seed,
                                       int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, int sto_mode,
                                       int64_t sto_value, int cfo_mode, double cfo_value, void* rx_out, uint8_t* ref_bits_out,
                                       uint8_t* sc_ref_bits_out, int64_t* sto_out, double* cfo_out, int flags) {
  const TxfImp imp(sto_mode, sto_value, cfo_mode, cfo_value);
  return txf_frames(pl, TxfCall("tx_frames_fused_ex", frame0, n_frames, scr_reg15).with_h(h, h_len).with_imp(sto_mode, cfo_mode),
                    snr_db, seed, &imp, TxfGenOut{rx_out, ref_bits_out, sc_ref_bits_out, sto_out, cfo_out, nullptr}, flags);
}

extern "C" int ofdm_tx_frames_fading_ex(ofdm_rx_plan* pl, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                        double snr_db, uint64_t seed, int64_t frame0, int64_t n_frames,
                                        const uint8_t* scr_reg15, int sto_mode, int64_t sto_value, int cfo_mode,
                                        double cfo_value, void* rx_out, uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out,
                                        double* taps_out, int64_t* sto_out, double* cfo_out, int flags) {
  const TxfImp imp(sto_mode, sto_value, cfo_mode, cfo_value);
  return txf_frames(pl, TxfCall("tx_frames_fading_ex", frame0, n_frames, scr_reg15)
                            .with_fading(tap_delay, tap_power, n_taps).with_imp(sto_mode, cfo_mode),
                    snr_db, seed, &imp, TxfGenOut{rx_out, ref_bits_out, sc_ref_bits_out, sto_out, cfo_out, taps_out}, flags);
}


// ofdm_tx_frames_fused_ex / ofdm_tx_frames_fading_ex in one entry (h, or the tap-delay line; both STO / CFO modes 0 and no
// sto_out / cfo_out: the plain channel pass of ofdm_tx_frames_fused / _fading) with the payload draw replaced by the caller's bits
extern "C" int ofdm_tx_frames_payload(ofdm_rx_plan* pl, const uint8_t* payload, int64_t n_bits, int64_t first_frame, const void* h,
                                      int h_len, const int32_t* tap_delay, const double* tap_power, int n_taps, double snr_db,
                                      uint64_t seed, int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, int sto_mode,
                                      int64_t sto_value, int cfo_mode, double cfo_value, void* rx_out, uint8_t* ref_bits_out,
                                      uint8_t* sc_ref_bits_out, double* taps_out, int64_t* sto_out, double* cfo_out, int flags) {
  const bool fading = tap_delay || tap_power || n_taps != 0;
  const TxfGivenBits given{payload, n_bits, first_frame, fading && h && h_len != 0};
  const TxfImp imp(sto_mode, sto_value, cfo_mode, cfo_value);
  const bool imp_on = sto_mode != 0 || cfo_mode != 0 || sto_out || cfo_out;
  TxfCall c("tx_frames_payload", frame0, n_frames, scr_reg15);
  c.with_imp(sto_mode, cfo_mode);
  if (fading) c.with_fading(tap_delay, tap_power, n_taps);
  else c.with_h(h, h_len);
  return txf_frames(pl, c, snr_db, seed, imp_on ? &imp : nullptr,
                    TxfGenOut{rx_out, ref_bits_out, sc_ref_bits_out, sto_out, cfo_out, fading ? taps_out : nullptr}, flags, &given);
}
