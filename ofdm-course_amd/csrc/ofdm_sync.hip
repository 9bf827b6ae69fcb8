// Receiver synchronisation, function by function: AutoCorrFunction (sliding CP autocorrelation + plateau search),
// remove_IFO, fine_sync.  Their kernels are in sync_core.hpp; the batched Task-4 receiver is ofdm_chain_t4.hip.
#include "sync_core.hpp"

namespace ofdm {

int demod_device(const void* y, void* x, int nfft, int64_t n_symb, int t_guard, bool f64);   // ofdm_modem.hip
int cfo_device(const void* y, void* out, int64_t len, double cfo, int nfft, bool f64);       // ofdm_channel.hip

// FreqOffset = -angle(AutoCorr(TgPosition)) / (2 pi) (AutoCorrFunction.m:27) of the plateau result resv = rho(TgPosition), into
// resv[2]: taken on the device by the expression of the batched routes (t4_scalars_kernel, t4_acf_search_kernel,
// sync_capture_kernel), so a frame has one FreqOffset whichever entry it goes through (the host's atan2 differs from the device's
// in the last place on some arguments)
__global__ void acf_freq_offset_kernel(double* __restrict__ resv) {
  resv[2] = -atan2(resv[1], resv[0]) / (2.0 * M_PI);
}

}  // namespace ofdm

using namespace ofdm;

extern "C" {

int ofdm_AutoCorrFunction(const void* rx, int64_t len, int width_window, int nfft, void* rho_out,
                          int64_t* tg_position_out, double* freq_offset_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(len >= 0 && width_window >= 1 && nfft >= 1, "AutoCorrFunction: bad sizes");
  OFDM_ARG(width_window <= ACF_MAXW, "AutoCorrFunction: WidthWindow %d exceeds the supported %d", width_window, ACF_MAXW);
  const bool f64 = is_f64(flags);
  const int64_t n_out = len - width_window - nfft;
  Stage st(flags);
  int64_t res[2] = {65, 0};
  double resv[3] = {NAN, NAN, NAN};                    // rho(TgPosition), FreqOffset
  if (n_out <= 0) {
    // zeros(1, <=0) -> empty AutoCorr; find() empty -> catch -> 65; AutoCorr(65) errors in MATLAB
    set_error("AutoCorrFunction: signal shorter than WidthWindow+Nfft (index exceeds array bounds at :27)");
    return OFDM_ERR_ARG;
  }
  const void* dx; void *drho, *dres, *dresv;
  OFDM_TRY(st.in(rx, csize(flags) * (size_t)len, &dx));
  if (rho_out) OFDM_TRY(st.out(rho_out, csize(flags) * (size_t)n_out, &drho));
  else OFDM_TRY(st.scratch(csize(flags) * (size_t)n_out, &drho));
  OFDM_TRY(st.fetch(res, sizeof(res), &dres));
  OFDM_TRY(st.fetch(resv, sizeof(resv), &dresv));
  const unsigned grid = cdiv_u(n_out, ACF_TILE);
  OFDM_TRY(f64 ? acf_prepare<double>() : acf_prepare<float>());
  if (f64) {
    hipLaunchKernelGGL(acf_kernel<double>, dim3(grid), dim3(ACF_THREADS), acf_lds_bytes<double>(width_window), ctx().stream, (const c64*)dx, len,
                       width_window, nfft, (c64*)drho, n_out);
    OFDM_TRY(check_launch("acf_kernel"));
    hipLaunchKernelGGL(acf_plateau_kernel<double>, dim3(1), dim3(PLAT_THREADS), 0, ctx().stream, (const c64*)drho,
                       n_out, width_window, 0.77, (int64_t*)dres, (double*)dresv);
  } else {
    hipLaunchKernelGGL(acf_kernel<float>, dim3(grid), dim3(ACF_THREADS), acf_lds_bytes<float>(width_window), ctx().stream, (const c32*)dx, len,
                       width_window, nfft, (c32*)drho, n_out);
    OFDM_TRY(check_launch("acf_kernel"));
    hipLaunchKernelGGL(acf_plateau_kernel<float>, dim3(1), dim3(PLAT_THREADS), 0, ctx().stream, (const c32*)drho,
                       n_out, width_window, 0.77, (int64_t*)dres, (double*)dresv);
  }
  OFDM_TRY(check_launch("acf_plateau_kernel"));
  hipLaunchKernelGGL(acf_freq_offset_kernel, dim3(1), dim3(1), 0, ctx().stream, (double*)dresv);
  OFDM_TRY(check_launch("acf_freq_offset_kernel"));
  OFDM_TRY(st.finish());
  if (tg_position_out) *tg_position_out = res[0];
  if (res[0] > n_out) {
    set_error("AutoCorrFunction: TgPosition %lld exceeds numel(AutoCorr)=%lld (index error at :27)",
              (long long)res[0], (long long)n_out);
    return OFDM_ERR_ARG;
  }
  if (freq_offset_out) *freq_offset_out = resv[2];                                         // :27
  return res[1] ? OFDM_OK : OFDM_SOFT_ACF_FALLBACK;
}

int ofdm_remove_IFO(const void* rx, int64_t len, int nfft, void* fixed_out, int* ifo_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(nfft >= 64 && (nfft & (nfft - 1)) == 0 && nfft <= 8192, "remove_IFO: unsupported Nfft %d", nfft);
  OFDM_ARG(len >= 2 * (int64_t)nfft, "remove_IFO: rx_signal(Nfft+1:2*Nfft) exceeds the signal length");
  const bool f64 = is_f64(flags);
  Stage st(flags);
  const void* dx; void *dout, *dspec, *dres;
  OFDM_TRY(st.in(rx, csize(flags) * (size_t)len, &dx));
  OFDM_TRY(st.out(fixed_out, csize(flags) * (size_t)len, &dout));
  OFDM_TRY(st.scratch(csize(flags) * (size_t)nfft, &dspec));
  int64_t first = -1;
  OFDM_TRY(st.scratch(sizeof(int64_t), &dres));
  // fft(rx(Nfft+1:2*Nfft)) : "symbol 0 with a guard of Nfft samples"   (remove_IFO.m:5)
  OFDM_TRY(demod_device(dx, dspec, nfft, 1, nfft, f64));
  if (f64) hipLaunchKernelGGL(first_above_kernel<double>, dim3(1), dim3(PLAT_THREADS), 0, ctx().stream, (const c64*)dspec, (int64_t)nfft, 0.77, (int64_t*)dres);
  else hipLaunchKernelGGL(first_above_kernel<float>, dim3(1), dim3(PLAT_THREADS), 0, ctx().stream, (const c32*)dspec, (int64_t)nfft, 0.77, (int64_t*)dres);
  OFDM_TRY(check_launch("first_above_kernel"));
  OFDM_HIP(hipMemcpyAsync(&first, dres, sizeof(first), hipMemcpyDeviceToHost, ctx().stream));
  OFDM_HIP(hipStreamSynchronize(ctx().stream));
  OFDM_ARG(first >= 0, "remove_IFO: no spectral line above 0.77 (inds(1) index error at :8)");
  if (ifo_out) *ifo_out = (int)first;                                        // inds(1)-1
  OFDM_TRY(cfo_device(dx, dout, len, -(double)first, nfft, f64));            // :9
  return st.finish();
}

int ofdm_fine_sync(const void* rx, int nfft, int64_t n_symb, const int32_t* pilot_carriers, int n_pilots,
                   const void* pilot_values, int time_desync, int freq_desync, int variant, void* out,
                   double* tau_out, double* phase_out, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(nfft > 0 && n_symb > 0 && n_pilots >= 2, "fine_sync: needs at least two pilot carriers");
  std::vector<int32_t> pc0(n_pilots);
  for (int i = 0; i < n_pilots; ++i) {
    OFDM_ARG(pilot_carriers[i] >= 1 && pilot_carriers[i] <= nfft, "fine_sync: pilot index outside 1..Nfft");
    pc0[i] = pilot_carriers[i] - 1;
  }
  const double deltak = (double)pilot_carriers[1] - (double)pilot_carriers[0];   // fine_sync.m:6
  const bool f64 = is_f64(flags);
  Stage st(flags);
  const void *dx, *dtx, *dpc; void *dout, *dest;
  OFDM_TRY(st.in(rx, csize(flags) * (size_t)nfft * n_symb, &dx));
  OFDM_TRY(st.in(pilot_values, csize(flags) * (size_t)n_pilots * n_symb, &dtx));
  OFDM_TRY(st.upload(pc0.data(), sizeof(int32_t) * n_pilots, &dpc));
  OFDM_TRY(st.out(out, csize(flags) * (size_t)nfft * n_symb, &dout));
  double est[2] = {0, 0};
  OFDM_TRY(st.fetch((tau_out || phase_out) ? est : nullptr, sizeof(est), &dest));
  const int64_t total = (int64_t)nfft * n_symb;
  if (f64) {
    PilotView<double> pv{(const c64*)dx, (const c64*)dtx, (const int32_t*)dpc, nfft, n_pilots, (int64_t)n_pilots * n_symb, 0, 0};
    hipLaunchKernelGGL(fine_tau_kernel<double>, dim3(1), dim3(FS_THREADS), 0, ctx().stream, pv, deltak, variant, (double*)dest);
    hipLaunchKernelGGL(fine_phase_kernel<double>, dim3(1), dim3(FS_THREADS), 0, ctx().stream, pv, time_desync, (double*)dest);
    hipLaunchKernelGGL(fine_apply_kernel<double>, dim3(ew_grid(total)), dim3(256), 0, ctx().stream, (const c64*)dx,
                       (c64*)dout, nfft, n_symb, time_desync, freq_desync, (const double*)dest);
  } else {
    PilotView<float> pv{(const c32*)dx, (const c32*)dtx, (const int32_t*)dpc, nfft, n_pilots, (int64_t)n_pilots * n_symb, 0, 0};
    hipLaunchKernelGGL(fine_tau_kernel<float>, dim3(1), dim3(FS_THREADS), 0, ctx().stream, pv, deltak, variant, (double*)dest);
    hipLaunchKernelGGL(fine_phase_kernel<float>, dim3(1), dim3(FS_THREADS), 0, ctx().stream, pv, time_desync, (double*)dest);
    hipLaunchKernelGGL(fine_apply_kernel<float>, dim3(ew_grid(total)), dim3(256), 0, ctx().stream, (const c32*)dx,
                       (c32*)dout, nfft, n_symb, time_desync, freq_desync, (const double*)dest);
  }
  OFDM_TRY(check_launch("fine_sync kernels"));
  OFDM_TRY(st.finish());
  if (tau_out) *tau_out = est[0];
  if (phase_out) *phase_out = est[1];
  return OFDM_OK;
}

}  // extern "C"
