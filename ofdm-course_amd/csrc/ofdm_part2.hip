// One (kk, jj-range) tile of Task 5/Task5_part2.m as a device-resident pass: the Monte-Carlo realisations jj of one pilot
// scenario kk share the noisy TX stream and differ in their channel (Task5_part2.m:148-205, :269-304).  Per realisation
//   conv(Tx_noised, h_jj) truncated                (:160-166)      fir_multi_kernel
//   OFDM_demodulator, rows 1..N_carrier            (:169-172)      demod_keep_device
//   Y = X(pilots, 1) ./ pilotValues(:, 1)          (:190)          p2_pilot_ls_kernel
//   LS_CE                                          (:174)          spline operator (interpolate.m) as ONE real GEMM over the tile
//   MMSE_CE(h = true CIR, SNR)                     (:176-177)      mmse_wave_kernel: one wavefront per realisation (Levinson),
//                                                                  then the same spline operator
//   MP_estimate                                    (:192)          mp_batch_kernel: S^H residue on the matrix cores per iteration
//   OMP_estimate                                   (:193)          omp_batch_kernel (ofdm_chain_fast.hip) while its state fits the LDS,
//                                                                  else omp_wide_kernel (ofdm_omp_wide.hip): omp_stage_run (chain_fast_core.hpp)
//   NMSE of the four estimates                     (:202-205)      p2_nmse_kernel against H = fft(h_jj)
//   equalize_signal -> get_payload -> demapping -> BER_func, four times (:269-304)   eq_demap_kernel (ofdm_chain_split.hip)
// Nothing returns to the host but 4 x n NMSE values and 4 x n error counts.
// From the demodulator to the four H buffers and the four error rows the stages are ONE body, est_body_run (est_body.hpp), that this
// tile, the MSE(SNR) tile below and the estimator study (ofdm_est_study.hip) call; each has its own front end and its own error
// kernel behind it.
#include <algorithm>

#include "est_body.hpp"
#include "mmse_levinson.hpp"
#include "mmse_tau.hpp"
#include "omp_wide_host.hpp"
#include "rx_plan.hpp"
#include "spline_op.hpp"

namespace ofdm {

int demod_keep_device(const void* y, void* x, int nfft, int64_t n_symb, int t_guard, int n_keep, bool f64);   // ofdm_modem.hip

// ---- conv(x, h_f.', 'full')(1:len) for every realisation f: sparse taps (delay, amplitude) per realisation
template <typename T>
__global__ void fir_multi_kernel(const cx<T>* __restrict__ x, int64_t len, const int32_t* __restrict__ delay,
                                 const c64* __restrict__ amp, int n_taps, cx<T>* __restrict__ out) {
  const int64_t f = blockIdx.y;
  const int32_t* d = delay + f * n_taps;
  const c64* a = amp + f * n_taps;
  for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < len; n += (int64_t)gridDim.x * blockDim.x) {
    double sr = 0, si = 0;
    for (int t = 0; t < n_taps; ++t) {
      const int64_t m = n - d[t];
      if (m >= 0) {
        const cx<T> v = x[m];
        sr += a[t].x * (double)v.x - a[t].y * (double)v.y;
        si += a[t].x * (double)v.y + a[t].y * (double)v.x;
      }
    }
    out[f * len + n] = mk<T>((T)sr, (T)si);
  }
}

template <typename T>
__global__ void p2_pilot_ls_kernel(const cx<T>* __restrict__ xk, const int32_t* __restrict__ pc0, const cx<T>* __restrict__ pilots,
                                   cx<T>* __restrict__ ypil, int np, int n_symb, int nc, int64_t n_frames) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_frames * np) return;
  const int64_t f = i / np;
  const int p = (int)(i - f * np);
  ypil[i] = cdiv(xk[f * n_symb * (int64_t)nc + pc0[p]], pilots[p]);
}

template <typename T>
__global__ void p2_replicate_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int words, int64_t n_frames) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_frames * words) dst[i] = src[i % words];
}

// ---- out[f][m] = sum_j W[m, j] v[f][j]: real operator [n_out x n_in] (column-major), P2_FT realisations per workgroup
constexpr int P2_FT = 8;
template <typename T>
__global__ __launch_bounds__(128) void p2_apply_operator_kernel(const double* __restrict__ W, const cx<T>* __restrict__ v,
                                                                cx<T>* __restrict__ out, int n_out, int n_in, int64_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p2_smem[];
  cx<T>* hs = (cx<T>*)p2_smem;                                     // [n_in][P2_FT]
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.y * P2_FT;
  for (int i = threadIdx.x; i < n_in * P2_FT; i += blockDim.x) {
    const int f = i / n_in, j = i - f * n_in;
    hs[j * P2_FT + f] = f0 + f < n_frames ? v[(f0 + f) * n_in + j] : mk<T>(0, 0);
  }
  __syncthreads();
  if (m >= n_out) return;
  double ar[P2_FT], ai[P2_FT];
#pragma unroll
  for (int f = 0; f < P2_FT; ++f) ar[f] = ai[f] = 0.0;
  for (int j0 = 0; j0 < n_in; j0 += 8) {
    double w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = j0 + u < n_in ? W[(size_t)(j0 + u) * n_out + m] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (j0 + u < n_in) {
#pragma unroll
        for (int f = 0; f < P2_FT; ++f) {
          const cx<T> z = hs[(j0 + u) * P2_FT + f];
          ar[f] += w[u] * (double)z.x;
          ai[f] += w[u] * (double)z.y;
        }
      }
  }
#pragma unroll
  for (int f = 0; f < P2_FT; ++f)
    if (f0 + f < n_frames) out[(f0 + f) * n_out + m] = mk<T>((T)ar[f], (T)ai[f]);
}

// ---- MMSE_CE.m:25-36 for one realisation per WAVEFRONT: mmse_toeplitz_wave (mmse_levinson.hpp), tau_rms of the realisation's CIR
// comes with it as c = 2 pi tau_rms df Nps
template <typename T>
__global__ __launch_bounds__(256) void mmse_wave_kernel(const cx<T>* __restrict__ ypil, const double* __restrict__ cvals,
                                                        double inv_snr, int np, cx<T>* __restrict__ vout, int64_t n_frames,
                                                        const double* __restrict__ inv_snr_v = nullptr) {
  // blockDim.x / 64 realisations per workgroup (4 while their state fits the LDS, fewer for many pilots);
  // inv_snr_v (optional): every realisation at its own SNR (the SNR sweep of Main_model_Task_5.m:305-315)
  extern __shared__ __attribute__((aligned(16))) unsigned char p2_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t f = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave;
  if (f >= n_frames) return;                                       // no workgroup barrier below
  if (inv_snr_v) inv_snr = inv_snr_v[f];
  c64* tcol = (c64*)p2_smem + (size_t)wave * 4 * np;               // [np] each: tcol, fv, bv, xv
  mmse_toeplitz_wave<T>(ypil + f * np, cvals[f], inv_snr, np, tcol, vout + f * np, lane);
}

// ---- MP_estimate.m:8-24 for a tile of realisations.  A workgroup of four wavefronts owns FB = 4 * fpw realisations:
//   per iteration  (1) C = S(:, 1:Np)^H * residue for all FB at once: fp32 on the matrix cores (v_mfma_f32_16x16x4_f32 through
//                      corr_mfma_f32; this is the dense product a random pilot mask needs, Task5_part2.m:58-64), else scalar
//                  (2) per realisation (a group of 64 / fpw lanes): projection |c|^2 / norm(a)^2 over the FIRST Np columns
//                      (:10), picked columns at -100 (:11-12), first maximum (:18), x = c(kp) / norm(a)^2 (:22),
//                      residue -= a_kp x (:21, :23)
// The picks / coefficients land in the plan's tap workspace, where the equalise stage turns them into H = fft(h) (:27-33).
struct MpLayout { unsigned off_r, off_c, off_pick, total; int fpw; };

template <typename T>
static MpLayout mp_layout(int np, int kc, int taps) {
  MpLayout o;
  int fpw = 4;
  auto bytes = [&](int f) { return sizeof(cx<T>) * (size_t)(4 * f) * (np + 1 + kc) + sizeof(int) * (size_t)(4 * f) * taps; };
  while (fpw > 1 && bytes(fpw) > 72 * 1024) fpw >>= 1;
  o.fpw = fpw;
  const int fb = 4 * fpw;
  unsigned b = 0;
  o.off_r = b;    b += (unsigned)((sizeof(cx<T>) * fb * (np + 1) + 15) & ~15u);
  o.off_c = b;    b += (unsigned)((sizeof(cx<T>) * fb * kc + 15) & ~15u);
  o.off_pick = b; b += (unsigned)((sizeof(int) * fb * taps + 15) & ~15u);
  o.total = b;
  return o;
}

template <typename T, bool MFMA>
__global__ __launch_bounds__(256) void mp_batch_kernel(FastParams<T> P, MpLayout lay, int kc, int64_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p2_smem[];
  cx<T>* Rl = (cx<T>*)(p2_smem + lay.off_r);      // [FB][np + 1] residue
  cx<T>* Cl = (cx<T>*)(p2_smem + lay.off_c);      // [FB][kc]     S^H residue
  int* picks = (int*)(p2_smem + lay.off_pick);    // [FB][taps]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int FPW = lay.fpw, FB = 4 * FPW;
  const int64_t f0 = (int64_t)blockIdx.x * FB;
  const int np = P.np, K = P.k_atoms, taps = P.taps, YS = np + 1;
  for (int i = tid; i < FB * np; i += 256) {
    const int f = i / np, p = i - f * np;
    Rl[f * YS + p] = (f0 + f < n_frames) ? P.ypil[(f0 + f) * np + p] : mk<T>(0, 0);
  }
  const int LPF = 64 / FPW, grp = lane / LPF, sl = lane - grp * LPF;
  const int fi = wave * FPW + grp;
  const int64_t f = f0 + fi;
  const bool live = f < n_frames;
  const double nrm2 = (double)np;                 // norm(a)^2 of a column of exp(-2 pi i ..): Np
  __syncthreads();
  for (int it = 0; it < taps; ++it) {
    // (1) correlations of every realisation of the workgroup
    if constexpr (MFMA) {
      corr_mfma_f32(P.sct, K, kc / 16, Rl, YS, np, FB, (float*)Cl, kc, wave, lane);
    } else {
      for (int i = tid; i < FB * kc; i += 256) {
        const int ff = i / kc, k = i - ff * kc;
        double ar = 0, ai = 0;
        for (int p = 0; p < np; ++p) {
          const cx<T> a = P.sct[(size_t)p * K + k], r = Rl[ff * YS + p];
          ar += (double)a.x * r.x - (double)a.y * r.y;
          ai += (double)a.x * r.y + (double)a.y * r.x;
        }
        Cl[i] = mk<T>((T)ar, (T)ai);
      }
    }
    __syncthreads();
    // (2) projection, first maximum over the group's lanes, update
    const cx<T>* cf = Cl + fi * kc;
    double bs = -1e300;
    int bi = 0x7fffffff;
    for (int k = sl; k < kc; k += LPF) {
      double sc = ((double)cf[k].x * cf[k].x + (double)cf[k].y * cf[k].y) / nrm2;
      for (int q = 0; q < it; ++q) if (picks[fi * taps + q] == k) sc = -100.0;
      if (sc > bs) { bs = sc; bi = k; }           // ascending k inside a lane: strict > keeps the first
    }
    double gm = bs;
    for (int off = LPF >> 1; off > 0; off >>= 1) gm = fmax(gm, __shfl_xor(gm, off, 64));
    int kp = bs == gm ? bi : 0x7fffffff;
    for (int off = LPF >> 1; off > 0; off >>= 1) kp = min(kp, __shfl_xor(kp, off, 64));
    if (kp >= kc) kp = 0;                         // all-NaN projections: MATLAB max returns index 1
    const cx<T> ck = cf[kp];
    const c64 x{(double)ck.x / nrm2, (double)ck.y / nrm2};
    cx<T>* rf = Rl + fi * YS;
    for (int p = sl; p < np; p += LPF) {
      const cx<T> a = conj(P.sct[(size_t)p * K + kp]);             // S(p, kp)
      const double rr = (double)rf[p].x - ((double)a.x * x.x - (double)a.y * x.y);
      const double ri = (double)rf[p].y - ((double)a.x * x.y + (double)a.y * x.x);
      rf[p] = mk<T>((T)rr, (T)ri);
    }
    if (sl == 0) {
      picks[fi * taps + it] = kp;
      if (live) {
        P.tap_idx[f * taps + it] = kp;
        P.tap_x[f * taps + it] = x;
        // h_impulse_est(kp(i1)) = x(i1) (:28-30): a later pick of the same column (possible once all Np columns are used
        // up: every projection is -100 and max returns column 1) overwrites the earlier coefficient
        for (int q = 0; q < it; ++q)
          if (picks[fi * taps + q] == kp) P.tap_x[f * taps + q] = c64{0, 0};
      }
    }
    __syncthreads();
  }
}

// ---- (H_f - H_est)(H_f - H_est)' / N_carrier for the four estimates (:202-205); H_f = fft(h_jj)(1..N_carrier) from the taps
template <typename T>
__global__ __launch_bounds__(256) void p2_nmse_kernel(const int32_t* __restrict__ delay, const c64* __restrict__ amp, int n_taps,
                                                      int nfft, int nc, const cx<T>* __restrict__ h0, const cx<T>* __restrict__ h1,
                                                      const cx<T>* __restrict__ h2, const cx<T>* __restrict__ h3,
                                                      double* __restrict__ nmse /* [4][n_frames] */, int64_t n_frames) {
  const int64_t f = blockIdx.x;
  __shared__ double red[4][4];
  double acc[4] = {0, 0, 0, 0};
  const cx<T>* hs[4] = {h0, h1, h2, h3};
  for (int k = threadIdx.x; k < nc; k += 256) {
    double hr = 0, hi = 0;
    for (int t = 0; t < n_taps; ++t) {
      const int e = (int)(((int64_t)delay[f * n_taps + t] * k) % nfft);
      double sn, cs;
      sincospi(2.0 * (double)e / (double)nfft, &sn, &cs);
      const c64 a = amp[f * n_taps + t];
      hr += a.x * cs + a.y * sn;                                   // a * exp(-2 pi i e / N)
      hi += a.y * cs - a.x * sn;
    }
#pragma unroll
    for (int e4 = 0; e4 < 4; ++e4) {
      const cx<T> he = hs[e4][f * nc + k];
      const double dr = hr - (double)he.x, di = hi - (double)he.y;
      acc[e4] += dr * dr + di * di;
    }
  }
#pragma unroll
  for (int e4 = 0; e4 < 4; ++e4) {
    double v = acc[e4];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[e4][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int e4 = threadIdx.x;
    nmse[e4 * n_frames + f] = (red[e4][0] + red[e4][1] + red[e4][2] + red[e4][3]) / (double)nc;
  }
}

template <typename T>
static int part2_tile_run(ofdm_rx_plan* pl, const void* dtx, const int32_t* ddelay, const c64* damp, int n_ch, int64_t F,
                          const double* dcvals, double inv_snr, const void* dref1, double* dnmse, uint32_t* derrs) {
  const int N = pl->nfft, nc = pl->n_carrier;
  const int64_t len = (int64_t)(N + pl->t_guard) * pl->n_symb;
  hipStream_t st = ctx().stream;
  // the front end's share of the arena: the realisations' frames and the reference bits of each
  const size_t o_ref = (sizeof(cx<T>) * (size_t)len * F + 255) & ~size_t(255);
  unsigned char *front, *body;
  OFDM_TRY(est_arena(pl, o_ref + (size_t)pl->frame_words * 4 * F, F, &front, &body));
  cx<T>* drx = (cx<T>*)front;
  uint32_t* dref = (uint32_t*)(front + o_ref);
  const EstBodyArgs a{"task5_part2_tile", 585, 585, dref, derrs, dcvals, inv_snr, nullptr};
  OFDM_TRY(est_body_check(pl, a.what, a.mmse_max_np, a.mmse_named_np, a.cvals == nullptr));
  // channel (:160-166); every realisation compares against the one reference
  hipLaunchKernelGGL(fir_multi_kernel<T>, dim3((unsigned)std::min<int64_t>((len + 255) / 256, 256), (unsigned)F), dim3(256), 0, st,
                     (const cx<T>*)dtx, len, ddelay, damp, n_ch, drx);
  OFDM_TRY(check_launch("fir_multi_kernel"));
  hipLaunchKernelGGL(p2_replicate_kernel<T>, dim3(cdiv_u(F * pl->frame_words, 256)), dim3(256), 0, st, (const uint32_t*)dref1, dref,
                     pl->frame_words, F);
  EstBodyOut<T> o;
  OFDM_TRY(est_body_run<T>(pl, a, drx, F, body, o));
  hipLaunchKernelGGL(p2_nmse_kernel<T>, dim3((unsigned)F), dim3(256), 0, st, ddelay, damp, n_ch, N, nc, (const cx<T>*)o.h[0],
                     (const cx<T>*)o.h[1], (const cx<T>*)o.h[2], (const cx<T>*)o.h[3], dnmse, F);
  return check_launch("p2_nmse_kernel");
}


// ---- MMSE_CE.m:18-25 with h = ifft(H_est_LS) (Main_model_Task_5.m:314-315): the N_carrier-point inverse DFT of the LS estimate
// (any N_carrier: direct sums over a table of the N_carrier-th roots of unity, exact index arithmetic), then
// hh = h h', r = sum(|h|^2 k) / hh, r2 = sum(|h|^2 k^2) / hh, tau_rms = sqrt(r2 - r^2); cvals[f] = 2 pi tau_rms df Nps.
template <typename T>
__global__ __launch_bounds__(256) void mse_tau_kernel(const cx<T>* __restrict__ hls, int nc, double nps, double* __restrict__ cvals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char p2_smem[];
  c64* const root = (c64*)p2_smem;                                  // exp(+2 pi i j / nc)
  c64* const hl = root + nc;                                        // the frame's H_est_LS in double
  __shared__ double red[3][4];
  const int64_t f = blockIdx.x;
  for (int j = threadIdx.x; j < nc; j += 256) {
    double sn, cs;
    sincospi(2.0 * (double)j / (double)nc, &sn, &cs);
    root[j] = c64{cs, sn};
    const cx<T> v = hls[f * nc + j];
    hl[j] = c64{(double)v.x, (double)v.y};
  }
  __syncthreads();
  double hh = 0, s1 = 0, s2 = 0;
  for (int k = threadIdx.x; k < nc; k += 256) {
    double ar = 0, ai = 0;
    int e = 0;                                                      // (k m) mod nc
    for (int m = 0; m < nc; ++m) {
      const c64 w = root[e], x = hl[m];
      ar += x.x * w.x - x.y * w.y;
      ai += x.x * w.y + x.y * w.x;
      e += k;
      if (e >= nc) e -= nc;
    }
    ar /= (double)nc; ai /= (double)nc;                             // ifft scaling
    const double p = ar * ar + ai * ai;
    hh += p; s1 += p * (double)k; s2 += p * (double)k * (double)k;
  }
  double v[3] = {hh, s1, s2};
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off, 64);
    if ((threadIdx.x & 63) == 0) red[q][threadIdx.x >> 6] = v[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double H = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    const double S1 = red[1][0] + red[1][1] + red[1][2] + red[1][3], S2 = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    cvals[f] = mmse_tau_c(H, S1, S2, 1.0 / (double)nc, nps);                            // :22-26, df = 1 / N_carrier
  }
}

// ---- H(1..N_carrier) = fft(h_est) from the picked taps of MP / OMP (MP_estimate.m:27-33, OMP_estimate.m:25-36): a later pick of
// the same atom overwrites the earlier one (est(index(i)) = x(i)).
template <typename T>
__global__ __launch_bounds__(256) void mse_taps_to_h_kernel(const int32_t* __restrict__ tap_idx, const c64* __restrict__ tap_x, int taps,
                                                            int nfft, int nc, cx<T>* __restrict__ hout) {
  const int64_t f = blockIdx.x;
  for (int k = threadIdx.x; k < nc; k += 256) {
    double hr = 0, hi = 0;
    for (int q = 0; q < taps; ++q) {
      const int idx = tap_idx[f * taps + q];
      if (idx < 0) continue;
      bool later = false;
      for (int q2 = q + 1; q2 < taps; ++q2) later = later || tap_idx[f * taps + q2] == idx;
      if (later) continue;
      const int e = (int)(((int64_t)idx * k) % nfft);
      double sn, cs;
      sincospi(2.0 * (double)e / (double)nfft, &sn, &cs);
      const c64 a = tap_x[f * taps + q];
      hr += a.x * cs + a.y * sn;
      hi += a.y * cs - a.x * sn;
    }
    hout[f * nc + k] = mk<T>((T)hr, (T)hi);
  }
}

// ---- the estimator body (est_body.hpp): its share of the arena, its refusals, its stages
struct EstBodyLayout {
  size_t o_x, o_v, o_c, o_h[4], total;
};

static EstBodyLayout est_body_layout(const ofdm_rx_plan* pl, int64_t F) {
  const size_t cs = pl->f64 ? sizeof(c64) : sizeof(c32), nc = (size_t)pl->n_carrier, nf = (size_t)F;
  EstBodyLayout l{};
  auto reserve = [&](size_t bytes) { const size_t o = l.total; l.total += (bytes + 255) & ~size_t(255); return o; };
  l.o_x = reserve(cs * nc * pl->n_symb * nf);
  l.o_v = reserve(cs * (size_t)pl->np * nf);
  l.o_c = reserve(sizeof(double) * nf);
  for (int e = 0; e < 4; ++e) l.o_h[e] = reserve(cs * nc * nf);
  return l;
}

size_t est_body_bytes(const ofdm_rx_plan* pl, int64_t F) { return est_body_layout(pl, F).total; }

int est_arena(ofdm_rx_plan* pl, size_t front, int64_t F, unsigned char** front_out, unsigned char** body_out) {
  front = (front + 255) & ~size_t(255);
  const size_t need = front + est_body_bytes(pl, F);
  if (pl->ws_t4_bytes < need) {                                     // the Task-4 arena doubles as these entries'
    OFDM_HIP(hipStreamSynchronize(ctx().stream));
    if (pl->ws_t4) { (void)hipFree(pl->ws_t4); pl->ws_t4 = nullptr; pl->ws_t4_bytes = 0; }
    OFDM_HIP(hipMalloc(&pl->ws_t4, need));
    pl->ws_t4_bytes = need;
  }
  *front_out = (unsigned char*)pl->ws_t4;
  *body_out = (unsigned char*)pl->ws_t4 + front;
  return OFDM_OK;
}

// wavefronts per workgroup of mmse_wave_kernel: 4 while their state fits the LDS, fewer for many pilots
static int mmse_wpw(int np) {
  int wpw = 4;
  while (wpw > 1 && sizeof(c64) * 4 * (size_t)np * wpw > 150 * 1024) wpw >>= 1;
  return wpw;
}

int est_body_check(const ofdm_rx_plan* pl, const char* what, int mmse_max_np, int mmse_named_np, bool ls_tau) {
  const int np = pl->np;
  if (ls_tau) OFDM_ARG(sizeof(c64) * 2 * (size_t)pl->n_carrier <= 150 * 1024, "%s: N_carrier beyond 4800", what);
  OFDM_ARG(np <= mmse_max_np, "%s: MMSE stage supports at most %d pilots", what, mmse_named_np);
  OFDM_ARG(pl->k_atoms >= np, "MP_estimate: the loop bound is Np columns (MP_estimate.m:10) but the dictionary has fewer");
  const unsigned mp_lds = pl->f64 ? mp_layout<double>(np, np, pl->taps).total : mp_layout<float>(np, np, pl->taps).total;
  OFDM_ARG(mp_lds <= 150 * 1024, "%s: MP stage needs %u bytes of LDS", what, mp_lds);
  return OFDM_OK;
}

template <typename T>
int est_body_run(ofdm_rx_plan* pl, const EstBodyArgs& a, const void* drx, int64_t F, unsigned char* body, EstBodyOut<T>& out) {
  const int N = pl->nfft, Tg = pl->t_guard, S = pl->n_symb, np = pl->np, nc = pl->n_carrier, taps = pl->taps;
  const bool f64 = std::is_same<T, double>::value;
  hipStream_t st = ctx().stream;
  OFDM_TRY(est_body_check(pl, a.what, a.mmse_max_np, a.mmse_named_np, a.cvals == nullptr));
  const EstBodyLayout l = est_body_layout(pl, F);
  cx<T>* dxk = (cx<T>*)(body + l.o_x);
  cx<T>* dv = (cx<T>*)(body + l.o_v);
  double* dcv = (double*)(body + l.o_c);
  cx<T>** dh = out.h;
  for (int e = 0; e < 4; ++e) dh[e] = (cx<T>*)(body + l.o_h[e]);
  // spline operator of interpolate.m (LS_CE.m:31, MMSE_CE.m:38): built once per plan, double
  if (!pl->d_p2_sop) {
    std::vector<double> W;
    OFDM_TRY(build_interpolate_operator(pl->pilot_loc.data(), np, nc, 's', W));
    OFDM_HIP(hipMalloc(&pl->d_p2_sop, sizeof(double) * W.size()));
    OFDM_HIP(hipMemcpy(pl->d_p2_sop, W.data(), sizeof(double) * W.size(), hipMemcpyHostToDevice));
  }
  FastPlanView pv;
  make_plan_view(pl, pv);
  pv.ev = nullptr;
  pv.d_wt = nullptr;
  pv.mmse_ls = 0;
  FastParams<T> P;
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(N, f64, &tw));
  OFDM_TRY(fast_params_prepare<T>(pv, tw, F, P));
  out.tap_idx = P.tap_idx;
  out.tap_x = P.tap_x;
  // demodulator, pilot LS values Y
  OFDM_TRY(demod_keep_device(drx, dxk, N, F * S, Tg, nc, f64));
  hipLaunchKernelGGL(p2_pilot_ls_kernel<T>, dim3(cdiv_u(F * np, 256)), dim3(256), 0, st, (const cx<T>*)dxk, (const int32_t*)pl->d_pc0,
                     (const cx<T>*)pl->d_pilots, P.ypil, np, S, nc, F);
  // LS_CE: H = Sop * Y
  const dim3 og(cdiv_u(nc, 128), cdiv_u(F, P2_FT));
  hipLaunchKernelGGL(p2_apply_operator_kernel<T>, og, dim3(128), sizeof(cx<T>) * np * P2_FT, st, (const double*)pl->d_p2_sop,
                     (const cx<T>*)P.ypil, dh[0], nc, np, F);
  // MMSE_CE: [tau_rms of ifft(H_est_LS),] v = rf2 (rf2 + I/snr)^-1 Y per frame, H = Sop * v
  {
    const double* cv = a.cvals;
    if (!cv) {
      const size_t tdyn = sizeof(c64) * 2 * (size_t)nc;
      OFDM_HIP(hipFuncSetAttribute((const void*)mse_tau_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tdyn));
      const double nps = (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0];                    // MMSE_CE.m:15
      hipLaunchKernelGGL(mse_tau_kernel<T>, dim3((unsigned)F), dim3(256), tdyn, st, (const cx<T>*)dh[0], nc, nps, dcv);
      cv = dcv;
    }
    const int wpw = mmse_wpw(np);
    const size_t dyn = sizeof(c64) * 4 * (size_t)np * wpw;
    OFDM_HIP(hipFuncSetAttribute((const void*)mmse_wave_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(mmse_wave_kernel<T>, dim3(cdiv_u(F, wpw)), dim3(64 * wpw), dyn, st, (const cx<T>*)P.ypil, cv, a.inv_snr, np, dv, F,
                       a.inv_snr_v);
    hipLaunchKernelGGL(p2_apply_operator_kernel<T>, og, dim3(128), sizeof(cx<T>) * np * P2_FT, st, (const double*)pl->d_p2_sop,
                       (const cx<T>*)dv, dh[1], nc, np, F);
  }
  OFDM_TRY(check_launch("LS / MMSE stage"));
  // MP_estimate: the picks and coefficients into the plan's tap workspace
  {
    const int kc = np;
    const MpLayout lay = mp_layout<T>(np, kc, taps);
    const unsigned grid = cdiv_u(F, 4 * lay.fpw);
    const bool mfma = !f64 && (kc % 16 == 0) && (np % 4 == 0) && !getenv("OFDM_MP_NO_MFMA");
    if (mfma) {
      if constexpr (!f64) {
        OFDM_HIP(hipFuncSetAttribute((const void*)mp_batch_kernel<float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.total));
        hipLaunchKernelGGL((mp_batch_kernel<float, true>), dim3(grid), dim3(256), lay.total, st, P, lay, kc, F);
      }
    } else {
      OFDM_HIP(hipFuncSetAttribute((const void*)mp_batch_kernel<T, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.total));
      hipLaunchKernelGGL((mp_batch_kernel<T, false>), dim3(grid), dim3(256), lay.total, st, P, lay, kc, F);
    }
    OFDM_TRY(check_launch("mp_batch_kernel"));
  }
  // The tap workspace holds one pursuit at a time, so MP's taps are turned into H before OMP_estimate overwrites them.  The body
  // ends in one of two tails.
  if (!a.ref) {
    // estimates only: H of MP and OMP is the transform of their taps
    auto taps_to_h = [&](cx<T>* h) {
      hipLaunchKernelGGL(mse_taps_to_h_kernel<T>, dim3((unsigned)F), dim3(256), 0, st, (const int32_t*)P.tap_idx, (const c64*)P.tap_x, taps, N,
                         nc, h);
    };
    taps_to_h(dh[2]);
    OFDM_TRY(omp_stage_run<T>(P, N, F));
    taps_to_h(dh[3]);
    return check_launch("mse_taps_to_h_kernel");
  }
  // with the equaliser: the equalise stage writes H of MP and OMP beside their bit errors; LS and MMSE are equalised with their H
  OFDM_TRY(eq_demap_run<T>(pv, P, dxk, nc, false, F, nullptr, a.ref, a.errs + 2 * F, dh[2], nullptr, nullptr, 0, 0));
  OFDM_TRY(omp_stage_run<T>(P, N, F));
  OFDM_TRY(eq_demap_run<T>(pv, P, dxk, nc, false, F, nullptr, a.ref, a.errs + 3 * F, dh[3], nullptr, nullptr, 0, 0));
  P.h_in = dh[0];
  OFDM_TRY(eq_demap_run<T>(pv, P, dxk, nc, true, F, nullptr, a.ref, a.errs + 0 * F, nullptr, nullptr, nullptr, 0, 0));
  P.h_in = dh[1];
  return eq_demap_run<T>(pv, P, dxk, nc, true, F, nullptr, a.ref, a.errs + 1 * F, nullptr, nullptr, nullptr, 0, 0);
}
template int est_body_run<float>(ofdm_rx_plan*, const EstBodyArgs&, const void*, int64_t, unsigned char*, EstBodyOut<float>&);
template int est_body_run<double>(ofdm_rx_plan*, const EstBodyArgs&, const void*, int64_t, unsigned char*, EstBodyOut<double>&);

template <typename T>
static int mse_tile_run(ofdm_rx_plan* pl, const void* dtx, const void* h_dense, int h_len, const int32_t* ddelay, const c64* damp,
                        int n_ch, const double* snr_db_host, const double* dinv_snr, int64_t F, uint64_t seed, uint32_t stream0,
                        double* dmse, int flags) {
  const int N = pl->nfft, nc = pl->n_carrier;
  const int64_t len = (int64_t)(N + pl->t_guard) * pl->n_symb;
  hipStream_t st = ctx().stream;
  const int devflags = (flags & ~OFDM_DEVICE) | OFDM_DEVICE;
  // the front end's share of the arena: the points' noisy frames, and the received ones
  const size_t o_b = (sizeof(cx<T>) * (size_t)len * F + 255) & ~size_t(255);
  unsigned char *front, *body;
  OFDM_TRY(est_arena(pl, 2 * o_b, F, &front, &body));
  cx<T>* da = (cx<T>*)front;
  cx<T>* db = (cx<T>*)(front + o_b);
  // no equaliser (:334-344 compare estimates only); tau_rms of ifft(H_est_LS), every point at its own SNR (:314-315)
  const EstBodyArgs a{"task5_mse_tile", 2400, 2343, nullptr, nullptr, nullptr, 0.0, dinv_snr};
  OFDM_TRY(est_body_check(pl, a.what, a.mmse_max_np, a.mmse_named_np, a.cvals == nullptr));
  // Tx for every point -> Noise at the point's SNR (:307) -> conv truncated (:308-309)
  const int words = (int)(len * (int64_t)(sizeof(cx<T>) / 4));
  OFDM_ARG((int64_t)words * F < ((int64_t)1 << 40), "task5_mse_tile: tile too large");
  hipLaunchKernelGGL(p2_replicate_kernel<T>, dim3(cdiv_u((int64_t)F * words, 256)), dim3(256), 0, st, (const uint32_t*)dtx, (uint32_t*)da,
                     words, F);
  OFDM_TRY(check_launch("p2_replicate_kernel"));
  OFDM_TRY(ofdm_Noise_frames_snr(snr_db_host, da, len, F, seed, stream0, da, devflags));
  OFDM_TRY(ofdm_channel_conv_frames(da, len, F, h_dense, h_len, db, devflags));
  EstBodyOut<T> o;
  OFDM_TRY(est_body_run<T>(pl, a, db, F, body, o));
  // the four errors against fft(h)(1..N_carrier) (:334-344)
  hipLaunchKernelGGL(p2_nmse_kernel<T>, dim3((unsigned)F), dim3(256), 0, st, ddelay, damp, n_ch, N, nc, (const cx<T>*)o.h[0],
                     (const cx<T>*)o.h[1], (const cx<T>*)o.h[2], (const cx<T>*)o.h[3], dmse, F);
  return check_launch("p2_nmse_kernel");
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_task5_part2_tile(ofdm_rx_plan* pl, const void* tx_noised, const int32_t* tap_delay, const double* tap_amp,
                                     int n_ch_taps, int64_t n_frames, double snr_db, const uint8_t* ref_bits, double* nmse_out,
                                     uint32_t* errors_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(!pl || !(pl->descr & DESCR_ON), "task5_part2_tile: the study runs unscrambled (Task5_part2.m:104-114,:285-299 are commented out); clear the plan's DeScrambler");
  OFDM_ARG(pl && tx_noised && tap_delay && tap_amp && ref_bits && nmse_out && errors_out, "task5_part2_tile: null argument");
  OFDM_ARG(pl->nd >= 1, "task5_part2_tile: the plan has no data carriers");
  OFDM_PLAN_DEVICE(pl);
  OFDM_ARG((is_f64(flags) ? 1 : 0) == pl->f64, "task5_part2_tile: precision flag differs from the plan's");
  OFDM_ARG(pl->pilots_in_band && pl->np >= 2, "task5_part2_tile: needs at least two pilots, all inside 1..N_carrier");
  OFDM_ARG(n_ch_taps >= 1 && n_ch_taps <= 64 && n_frames >= 0 && n_frames <= 65535, "task5_part2_tile: 1..64 channel taps, at most 65535 realisations");
  OFDM_ARG(chain_split_fits(pl->taps, pl->bps, pl->n_carrier, (int64_t)pl->nd * pl->n_symb, pl->f64 != 0),
           "task5_part2_tile: the frame's decisions do not fit the equalise stage's LDS");
  if (n_frames == 0) return OFDM_OK;
  const size_t cs = csize(flags);
  const int64_t len = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  // rms delay spread of every realisation's CIR (MMSE_CE.m:19-24 on h_t(1:N_carrier), Task5_part2.m:176) -> c = 2 pi tau df Nps
  std::vector<double> cvals((size_t)n_frames);
  const double nps = (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0], df = 1.0 / (double)pl->n_carrier;   // MMSE_CE.m:15, :25
  for (int64_t f = 0; f < n_frames; ++f) {
    double hh = 0, s1 = 0, s2 = 0;
    for (int t = 0; t < n_ch_taps; ++t) {
      const int d = tap_delay[f * n_ch_taps + t];
      OFDM_ARG(d >= 0 && d < pl->nfft, "task5_part2_tile: tap delay outside 0..Nfft-1");
      if (d >= pl->n_carrier) continue;                            // h_t(1:N_carrier)
      const double ar = tap_amp[2 * (f * n_ch_taps + t)], ai = tap_amp[2 * (f * n_ch_taps + t) + 1];
      const double p = ar * ar + ai * ai;
      hh += p; s1 += p * d; s2 += p * (double)d * d;
    }
    OFDM_ARG(hh > 0, "task5_part2_tile: impulse response of realisation %lld is all zero inside 1..N_carrier", (long long)f);
    cvals[f] = mmse_tau_c(hh, s1, s2, df, nps);                    // (one path: r2 - r^2 clamped at 0)
  }
  Stage st(flags);
  const void *dtx, *ddel, *damp, *dcv, *dref;
  void *dnm, *der;
  OFDM_TRY(st.in(tx_noised, cs * (size_t)len, &dtx));
  OFDM_TRY(st.upload(tap_delay, sizeof(int32_t) * (size_t)n_frames * n_ch_taps, &ddel));
  OFDM_TRY(st.upload(tap_amp, sizeof(double) * 2 * (size_t)n_frames * n_ch_taps, &damp));
  OFDM_TRY(st.upload(cvals.data(), sizeof(double) * (size_t)n_frames, &dcv));
  OFDM_TRY(st.in(ref_bits, (size_t)pl->frame_words * 4, &dref));
  OFDM_TRY(st.out(nmse_out, sizeof(double) * 4 * (size_t)n_frames, &dnm));
  OFDM_TRY(st.out(errors_out, sizeof(uint32_t) * 4 * (size_t)n_frames, &der));
  const double inv_snr = 1.0 / pow(10.0, snr_db * 0.1);            // MMSE_CE.m:13
  if (pl->f64) OFDM_TRY(part2_tile_run<double>(pl, dtx, (const int32_t*)ddel, (const c64*)damp, n_ch_taps, n_frames, (const double*)dcv,
                                                inv_snr, dref, (double*)dnm, (uint32_t*)der));
  else OFDM_TRY(part2_tile_run<float>(pl, dtx, (const int32_t*)ddel, (const c64*)damp, n_ch_taps, n_frames, (const double*)dcv, inv_snr,
                                      dref, (double*)dnm, (uint32_t*)der));
  return st.finish();
}

__global__ void omp_index_out_kernel(const int32_t* __restrict__ tap_idx, int32_t* __restrict__ index_out, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) index_out[i] = tap_idx[i] + 1;                    // 1-based, 0 = unused
}

template <typename T>
static int omp_estimate_batch_run(ofdm_rx_plan* pl, const void* dy, int64_t n, int route, int32_t* didx, c64* dx, void* dh) {
  hipStream_t st = ctx().stream;
  FastPlanView pv;
  make_plan_view(pl, pv);
  pv.ev = nullptr;
  pv.d_wt = nullptr;
  pv.mmse_ls = 0;
  FastParams<T> P;
  const void* tw = nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &tw));
  OFDM_TRY(fast_params_prepare<T>(pv, tw, n, P));
  OFDM_HIP(hipMemcpyAsync(P.ypil, dy, sizeof(cx<T>) * (size_t)pl->np * n, hipMemcpyDeviceToDevice, st));
  OFDM_TRY(omp_stage_run<T>(P, pl->nfft, n, route));
  const int64_t count = (int64_t)pl->taps * n;
  hipLaunchKernelGGL(omp_index_out_kernel, dim3(cdiv_u(count, 256)), dim3(256), 0, st, (const int32_t*)P.tap_idx, didx, count);
  OFDM_HIP(hipMemcpyAsync(dx, P.tap_x, sizeof(c64) * (size_t)count, hipMemcpyDeviceToDevice, st));
  if (dh)
    hipLaunchKernelGGL(mse_taps_to_h_kernel<T>, dim3((unsigned)n), dim3(256), 0, st, (const int32_t*)P.tap_idx, (const c64*)P.tap_x,
                       pl->taps, pl->nfft, pl->n_carrier, (cx<T>*)dh);
  return check_launch("OMP_estimate_batch");
}

extern "C" int ofdm_OMP_estimate_batch(ofdm_rx_plan* pl, const void* y, int64_t n, int route, int32_t* index_out, void* x_out,
                                       void* h_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && y && index_out && x_out, "OMP_estimate_batch: null argument");
  OFDM_PLAN_DEVICE(pl);
  OFDM_ARG((is_f64(flags) ? 1 : 0) == pl->f64, "OMP_estimate_batch: precision flag differs from the plan's");
  OFDM_ARG(n >= 0 && n <= 65535, "OMP_estimate_batch: at most 65535 realisations");
  OFDM_ARG(route == OMP_ROUTE_AUTO || route == OMP_ROUTE_BATCH || route == OMP_ROUTE_WIDE,
           "OMP_estimate_batch: route must be 0 (library's choice), 1 (omp_batch_kernel) or 2 (wide)");
  if (n == 0) return OFDM_OK;
  const size_t cs = csize(flags);
  Stage st(flags);
  const void* dy;
  void *didx, *dx, *dh = nullptr;
  OFDM_TRY(st.in(y, cs * (size_t)pl->np * n, &dy));
  OFDM_TRY(st.out(index_out, sizeof(int32_t) * (size_t)pl->taps * n, &didx));
  OFDM_TRY(st.out(x_out, sizeof(c64) * (size_t)pl->taps * n, &dx));
  if (h_out) OFDM_TRY(st.out(h_out, cs * (size_t)pl->n_carrier * n, &dh));
  if (pl->f64) OFDM_TRY(omp_estimate_batch_run<double>(pl, dy, n, route, (int32_t*)didx, (c64*)dx, dh));
  else OFDM_TRY(omp_estimate_batch_run<float>(pl, dy, n, route, (int32_t*)didx, (c64*)dx, dh));
  return st.finish();
}

extern "C" int ofdm_task5_mse_tile(ofdm_rx_plan* pl, const void* tx, const int32_t* tap_delay, const double* tap_amp, int n_ch_taps,
                                   const double* snr_db, int64_t n_points, uint64_t seed, uint32_t stream0, double* mse_out,
                                   int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && tx && tap_delay && tap_amp && snr_db && mse_out, "task5_mse_tile: null argument");
  OFDM_PLAN_DEVICE(pl);
  OFDM_ARG((is_f64(flags) ? 1 : 0) == pl->f64, "task5_mse_tile: precision flag differs from the plan's");
  OFDM_ARG(pl->pilots_in_band && pl->np >= 2, "task5_mse_tile: needs at least two pilots, all inside 1..N_carrier");
  OFDM_ARG(n_ch_taps >= 1 && n_ch_taps <= 64 && n_points >= 0 && n_points <= 65535, "task5_mse_tile: 1..64 channel taps, at most 65535 points");
  OFDM_ARG((int64_t)stream0 + n_points < ((int64_t)1 << 32), "task5_mse_tile: stream index outside 32 bits");
  if (n_points == 0) return OFDM_OK;
  const size_t cs = csize(flags);
  const int64_t len = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  // dense impulse response for conv (get_MP_channel_resp.m: amplitudes at their delays), the channel per point for the error
  // kernel, 1 / snr per point (MMSE_CE.m:13)
  int h_len = 0;
  for (int t = 0; t < n_ch_taps; ++t) {
    OFDM_ARG(tap_delay[t] >= 0 && tap_delay[t] < pl->nfft, "task5_mse_tile: tap delay outside 0..Nfft-1");
    h_len = std::max(h_len, tap_delay[t] + 1);
  }
  std::vector<c64> h64((size_t)h_len, c64{0, 0});
  for (int t = 0; t < n_ch_taps; ++t) h64[tap_delay[t]] = c64{tap_amp[2 * t], tap_amp[2 * t + 1]};   // a later tap at the same delay wins
  std::vector<c32> h32;
  const void* h_dense = h64.data();
  if (!pl->f64) {
    h32.resize(h64.size());
    for (size_t i = 0; i < h64.size(); ++i) h32[i] = c32{(float)h64[i].x, (float)h64[i].y};
    h_dense = h32.data();
  }
  std::vector<int32_t> del((size_t)n_points * n_ch_taps);
  std::vector<double> amp(2 * (size_t)n_points * n_ch_taps), inv_snr((size_t)n_points);
  for (int64_t f = 0; f < n_points; ++f) {
    for (int t = 0; t < n_ch_taps; ++t) {
      // the dense vector is what the script convolves with: the error is measured against ITS transform
      del[f * n_ch_taps + t] = tap_delay[t];
      const c64 a = h64[tap_delay[t]];
      bool dup = false;
      for (int t2 = t + 1; t2 < n_ch_taps; ++t2) dup = dup || tap_delay[t2] == tap_delay[t];
      amp[2 * (f * n_ch_taps + t)] = dup ? 0.0 : a.x;
      amp[2 * (f * n_ch_taps + t) + 1] = dup ? 0.0 : a.y;
    }
    inv_snr[f] = 1.0 / pow(10.0, snr_db[f] * 0.1);
  }
  Stage st(flags);
  const void *dtx, *ddel, *damp, *dinv;
  void* dms;
  OFDM_TRY(st.in(tx, cs * (size_t)len, &dtx));
  OFDM_TRY(st.upload(del.data(), sizeof(int32_t) * del.size(), &ddel));
  OFDM_TRY(st.upload(amp.data(), sizeof(double) * amp.size(), &damp));
  OFDM_TRY(st.upload(inv_snr.data(), sizeof(double) * inv_snr.size(), &dinv));
  OFDM_TRY(st.out(mse_out, sizeof(double) * 4 * (size_t)n_points, &dms));
  if (pl->f64) OFDM_TRY(mse_tile_run<double>(pl, dtx, h_dense, h_len, (const int32_t*)ddel, (const c64*)damp, n_ch_taps, snr_db,
                                              (const double*)dinv, n_points, seed, stream0, (double*)dms, flags));
  else OFDM_TRY(mse_tile_run<float>(pl, dtx, h_dense, h_len, (const int32_t*)ddel, (const c64*)damp, n_ch_taps, snr_db, (const double*)dinv,
                                    n_points, seed, stream0, (double*)dms, flags));
  return st.finish();
}
