// The OMP route of an RX plan (ofdm_rx_plan_set_omp_route): which kernel runs the OMP stage of ofdm_rx_chain_task5(_ex) and of the
// Task-5 BER sweeps, which all go through rx_chain_task5_run (ofdm_chain.hip).
//   OMP_ROUTE_BATCH  (a new plan) omp_batch_kernel, or the fused symbol-1 + OMP launch where the plan takes it: nothing changes
//   OMP_ROUTE_AUTO   the same wherever omp_batch_kernel's state fits the LDS (fused launch included, bit-identical); else
//                    rx_pilot_kernel / the split form's pilot stage -> omp_wide_kernel (ofdm_omp_wide.hip) -> the symbol stage
//   OMP_ROUTE_WIDE   always the three-launch form with omp_wide_kernel
// A shape the chosen kernel cannot serve is an argument error before anything is launched, never a fallback.  The dispatch itself
// is omp_stage_run (chain_fast_core.hpp) at the three call sites of the receiver; the MMSE modes have no OMP stage and ignore the
// route.
#include "rx_plan.hpp"

namespace ofdm {

int omp_route_check(const FastPlanView& pv) {
  if (pv.omp_out) *pv.omp_out = pv.mmse() ? 0 : OMP_ROUTE_BATCH;      // (the fused launch is a batch pursuit; omp_stage_run overwrites)
  if (pv.mmse() || pv.omp_route == OMP_ROUTE_BATCH) return OFDM_OK;
  unsigned lds;
  if (pv.f64) {
    FastParams<double> P{};
    P.np = pv.np; P.k_atoms = pv.k_atoms; P.taps = pv.taps; P.comb_m = pv.comb_m;
    lds = omp_batch_lds_bytes<double>(P);
  } else {
    FastParams<float> P{};
    P.np = pv.np; P.k_atoms = pv.k_atoms; P.taps = pv.taps; P.comb_m = pv.comb_m;
    lds = omp_batch_lds_bytes<float>(P);
  }
  const char* why = nullptr;
  const int r = omp_route_choose(pv.omp_route, lds, pv.nfft, pv.k_atoms, pv.taps, &why);
  OFDM_ARG(r != 0, "rx_chain_task5: %s", why);
  return OFDM_OK;
}

int omp_route_check_generic(ofdm_rx_plan* pl) {
  pl->last_omp = 0;
  OFDM_ARG(pl->omp_route != OMP_ROUTE_WIDE,
           "rx_chain_task5: the wide OMP route needs the three-launch receiver (Nfft 512, 1024, 2048 or 4096, pilots inside "
           "1..N_carrier); this plan takes the generic single-kernel entry (Nfft %d, %s), which runs its own pursuit",
           pl->nfft, pl->pilots_in_band ? "pilots in band" : "a pilot outside 1..N_carrier");
  return OFDM_OK;
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_rx_plan_set_omp_route(ofdm_rx_plan* pl, int route) {
  OFDM_ARG(pl, "rx_plan_set_omp_route: null plan");
  OFDM_ARG(route == OMP_ROUTE_AUTO || route == OMP_ROUTE_BATCH || route == OMP_ROUTE_WIDE,
           "rx_plan_set_omp_route: route must be 0 (library's choice), 1 (omp_batch_kernel) or 2 (wide)");
  pl->omp_route = route;
  return OFDM_OK;
}

extern "C" int ofdm_rx_plan_get_omp_route(const ofdm_rx_plan* pl, int* route_out, int* last_out) {
  OFDM_ARG(pl, "rx_plan_get_omp_route: null plan");
  if (route_out) *route_out = pl->omp_route;
  if (last_out) *last_out = pl->last_omp;
  return OFDM_OK;
}
