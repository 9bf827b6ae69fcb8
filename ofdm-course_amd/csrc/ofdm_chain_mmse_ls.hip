// MMSE mode of the fused RX chain WITHOUT a supplied channel (ofdm_rx_plan_set_mmse_ls): per frame
//   H_LS = LS_CE(Y, Xp, pilot_loc, N_carrier);  h = ifft(H_LS);  H = MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR)
// as T5/Main_model_Task_5.m:178-180 and :317-319 call it -- the rms delay spread comes from the frame itself, so nothing of
// the estimator but the spline operator is shared between frames.  From the pilot LS values y of symbol 1 (P.ypil):
//   (a) MMSE_CE.m:19-26.  H_LS = W y (W = interpolate.m as a real operator), so the three sums sum_k k^q |h_k|^2 are the
//       Hermitian forms y^H A_q y with A_q [Np x Np] built once per plan (mmse_ls_forms.hpp): 3 Np^2 multiply-adds per frame, no
//       N_carrier-point transform.  r2 - r^2 cancels, so the sums are double on fp32 plans too, and the difference is clamped at 0.
//   (b) MMSE_CE.m:30-36.  z = (rf2 + I/snr) \ y, v = rf2 z: the Levinson recursion of mmse_levinson.hpp, one wavefront per frame.
//   (c) MMSE_CE.m:38.  H = interpolate(v): the banded spline product on fp32 plans, the dense operator on fp64 plans.
// Every sum has a fixed order and a frame touches no other frame's data: the result does not depend on the batch it came in.
#include <algorithm>
#include <vector>

#include "mmse_levinson.hpp"
#include "mmse_ls_forms.hpp"
#include "mmse_tau.hpp"
#include "rx_plan.hpp"
#include "spline_op.hpp"

namespace ofdm {

constexpr int LS_MAX_WPW = 4;                                  // frames (= wavefronts) per workgroup

// One workgroup = blockDim.x / 64 frames.  Phase 1, all threads: thread t takes the rows t, t + blockDim.x, .. of the three
// forms and applies each loaded A_q(i, j) to every frame of the workgroup (the forms are read once per workgroup, not once per
// frame); the partial sums are reduced over the wavefront by shuffles and over the workgroup in wavefront order.  Phase 2, one
// wavefront per frame: c = 2 pi tau_rms df Nps and the Toeplitz solve.
template <typename T>
__global__ __launch_bounds__(256) void mmse_ls_wave_kernel(const cx<T>* __restrict__ ypil, const c64* __restrict__ aq, double cscale,
                                                           double inv_snr, int np, cx<T>* __restrict__ vout, int64_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ls_smem[];
  __shared__ double red[LS_MAX_WPW][3][LS_MAX_WPW];            // [wavefront][q][frame]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wpw = blockDim.x >> 6;
  const int64_t f0 = (int64_t)blockIdx.x * wpw;
  c64* const yd = (c64*)ls_smem;                               // [wpw][np]: the pilot LS values in double
  c64* const lev = yd + (size_t)wpw * np;                      // [wpw][4 np]: Levinson state per wavefront
  for (int i = tid; i < wpw * np; i += blockDim.x) {
    const int w = i / np;
    const cx<T> v = f0 + w < n_frames ? ypil[f0 * np + i] : mk<T>(0, 0);
    yd[i] = c64{(double)v.x, (double)v.y};
  }
  __syncthreads();
  double s[3][LS_MAX_WPW];
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int w = 0; w < LS_MAX_WPW; ++w) s[q][w] = 0.0;
  const size_t plane = (size_t)np * np;
  for (int i = tid; i < np; i += blockDim.x) {
    c64 u[3][LS_MAX_WPW];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int w = 0; w < LS_MAX_WPW; ++w) u[q][w] = c64{0, 0};
    for (int j = 0; j < np; ++j) {
      const size_t e = (size_t)j * np + i;                     // A_q(i, j): consecutive rows in consecutive lanes
      const c64 a0 = aq[e], a1 = aq[plane + e], a2 = aq[2 * plane + e];
#pragma unroll
      for (int w = 0; w < LS_MAX_WPW; ++w)
        if (w < wpw) {
          const c64 yj = yd[w * np + j];
          u[0][w] = u[0][w] + a0 * yj;
          u[1][w] = u[1][w] + a1 * yj;
          u[2][w] = u[2][w] + a2 * yj;
        }
    }
#pragma unroll
    for (int w = 0; w < LS_MAX_WPW; ++w)
      if (w < wpw) {
        const c64 yi = yd[w * np + i];
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q][w] += yi.x * u[q][w].x + yi.y * u[q][w].y;      // Re(conj(y_i) u_i)
      }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q)
#pragma unroll
    for (int w = 0; w < LS_MAX_WPW; ++w) {
      const double t = p2_wave_sum(s[q][w]);
      if (lane == 0) red[wave][q][w] = t;
    }
  __syncthreads();
  const int64_t f = f0 + wave;
  if (f >= n_frames) return;                                   // no workgroup barrier below
  double m[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    double t = 0.0;
    for (int w = 0; w < wpw; ++w) t += red[w][q][wave];
    m[q] = t;
  }
  const double c = cscale * mmse_tau_rms(m[0], m[1], m[2]);    // MMSE_CE.m:20-26,:30 (a one-tap channel: r2 - r^2 clamped at 0)
  mmse_toeplitz_wave<T>(ypil + f * np, c, inv_snr, np, lev + (size_t)wave * 4 * np, vout + f * np, lane);
}

template <typename T>
int mmse_ls_stage_run(const FastPlanView& pv, const FastParams<T>& P, int64_t n_frames) {
  const int np = pv.np;
  hipStream_t st = ctx().stream;
  const size_t need = sizeof(cx<T>) * (size_t)np * n_frames;
  if (!*pv.ws_lsv || *pv.ws_lsv_bytes < need) {
    OFDM_HIP(hipStreamSynchronize(st));
    if (*pv.ws_lsv) { (void)hipFree(*pv.ws_lsv); *pv.ws_lsv = nullptr; *pv.ws_lsv_bytes = 0; }
    OFDM_HIP(hipMalloc(pv.ws_lsv, need));
    *pv.ws_lsv_bytes = need;
  }
  int wpw = LS_MAX_WPW;
  auto bytes = [&](int w) { return sizeof(c64) * 5 * (size_t)np * w; };
  while (wpw > 1 && bytes(wpw) > 150 * 1024) wpw >>= 1;
  const size_t dyn = bytes(wpw);
  OFDM_ARG(dyn <= 150 * 1024, "rx_chain_task5 (MMSE mode, h = ifft(H_LS)): %d pilots do not fit the LDS", np);
  // (set on every launch: the attribute is kept per device, and beyond 64 KB the launch fails without it)
  OFDM_HIP(hipFuncSetAttribute((const void*)mmse_ls_wave_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
  hipLaunchKernelGGL(mmse_ls_wave_kernel<T>, dim3(cdiv_u(n_frames, wpw)), dim3(64 * wpw), dyn, st, (const cx<T>*)P.ypil,
                     (const c64*)pv.d_ls_aq, pv.ls_cscale, pv.ls_inv_snr, np, (cx<T>*)*pv.ws_lsv, n_frames);
  OFDM_TRY(check_launch("mmse_ls_wave_kernel"));
  if constexpr (std::is_same<T, float>::value) {
    const int rc = spline_band_run(pv.d_ls_bw, pv.d_ls_bc0, pv.ls_bw, pv.ls_span, *pv.ws_lsv, *pv.ws_h, np, pv.n_carrier, n_frames);
    OFDM_ARG(rc <= 0, "rx_chain_task5 (MMSE mode, h = ifft(H_LS)): the spline band does not fit the LDS");
    return rc;
  } else {
    return mmse_apply_run<T>(pv.d_ls_wt, *pv.ws_lsv, *pv.ws_h, np, pv.ls_m_pad, pv.n_carrier, n_frames);
  }
}
template int mmse_ls_stage_run<float>(const FastPlanView&, const FastParams<float>&, int64_t);
template int mmse_ls_stage_run<double>(const FastPlanView&, const FastParams<double>&, int64_t);

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_plan_set_mmse_ls(ofdm_rx_plan* pl, int enable, double snr_db) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl, "rx_plan_set_mmse_ls: null plan");
  OFDM_PLAN_DEVICE(pl);
  if (!enable) {                                                // back to OMP mode, as ofdm_rx_plan_set_mmse(h = NULL)
    OFDM_TRY(ofdm_rx_plan_set_mmse(pl, nullptr, 0, 0.0, 0));
    pl->mmse_ls = 0;
    return OFDM_OK;
  }
  const int np = pl->np, nc = pl->n_carrier;
  OFDM_ARG(np >= 2 && np <= 512, "rx_plan_set_mmse_ls: 2..512 pilots supported (the forms are built on the host)");
  OFDM_ARG(pl->pilots_in_band, "rx_plan_set_mmse_ls: the pilots must lie inside 1..N_carrier");
  if (!pl->d_ls_aq) {                                           // the plan's geometry is fixed: built once
    std::vector<double> sop;                                    // [nc x np], column-major
    OFDM_TRY(build_interpolate_operator(pl->pilot_loc.data(), np, nc, 's', sop));
    std::vector<ls_zc> aq;
    build_ls_moment_forms(sop.data(), nc, np, aq);
    static_assert(sizeof(ls_zc) == sizeof(c64), "std::complex<double> is two doubles");
    void *d_aq = nullptr, *d_wt = nullptr, *d_bw = nullptr, *d_bc0 = nullptr;
    int bw = 0, span = 0;
    const int m_pad = (nc + 15) & ~15;
    auto fail = [&](int rc) {
      for (void* q : {d_aq, d_wt, d_bw, d_bc0}) if (q) (void)hipFree(q);
      return rc;
    };
    auto to_dev = [&](const void* src, size_t n_bytes, void** dst) -> int {
      OFDM_HIP(hipMalloc(dst, n_bytes));
      OFDM_HIP(hipMemcpy(*dst, src, n_bytes, hipMemcpyHostToDevice));
      return OFDM_OK;
    };
    int rc = to_dev(aq.data(), sizeof(c64) * aq.size(), &d_aq);
    if (rc == OFDM_OK && pl->f64) {                             // the dense operator, as the fixed-h mode applies it
      std::vector<c64> wt((size_t)np * m_pad, c64{0, 0});
      for (int j = 0; j < np; ++j)
        for (int m = 0; m < nc; ++m) wt[(size_t)j * m_pad + m] = c64{sop[m + (size_t)j * nc], 0.0};
      rc = to_dev(wt.data(), sizeof(c64) * wt.size(), &d_wt);
    } else if (rc == OFDM_OK) {
      std::vector<float> w;
      std::vector<int32_t> c0;
      mmse_band_spline(sop, nc, np, w, c0, bw, span);
      if (spline_band_lds_bytes(bw, span) > 150 * 1024) {          // refused here, not at the first chain call
        (void)fail(OFDM_ERR_ARG);
        OFDM_ARG(false, "rx_plan_set_mmse_ls: the spline band of this pilot layout needs %zu bytes of LDS (use an fp64 plan)",
                 spline_band_lds_bytes(bw, span));
      }
      rc = to_dev(w.data(), sizeof(float) * w.size(), &d_bw);
      if (rc == OFDM_OK) rc = to_dev(c0.data(), sizeof(int32_t) * c0.size(), &d_bc0);
    }
    if (rc != OFDM_OK) return fail(rc);
    pl->d_ls_aq = d_aq; pl->d_ls_wt = d_wt; pl->d_ls_bw = d_bw; pl->d_ls_bc0 = d_bc0;
    pl->ls_m_pad = m_pad; pl->ls_bw = bw; pl->ls_span = span;
    const double nps = (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0];          // MMSE_CE.m:15
    pl->ls_cscale = 2.0 * M_PI * (1.0 / (double)nc) * nps;                           // :25-26,:30
  }
  OFDM_TRY(ofdm_rx_plan_set_mmse(pl, nullptr, 0, 0.0, 0));      // the fixed-h mode off
  pl->ls_snr_db = snr_db;
  pl->ls_inv_snr = 1.0 / std::pow(10.0, snr_db * 0.1);          // MMSE_CE.m:13
  pl->mmse_ls = 1;
  return OFDM_OK;
}
