// The OMP route of an RX plan (ofdm_rx_plan_set_omp_route): which kernel runs the OMP stage of ofdm_rx_chain_task5(_ex) and of the
// Task-5 BER sweeps, which all go through rx_chain_task5_run (ofdm_chain.hip).
//   OMP_ROUTE_BATCH  (a new plan) omp_batch_kernel, or the fused symbol-1 + OMP launch where the plan takes it: nothing changes
//   OMP_ROUTE_AUTO   the same wherever omp_batch_kernel's state fits the LDS (fused launch included, bit-identical); else
//                    rx_pilot_kernel / the split form's pilot stage -> omp_wide_kernel (ofdm_omp_wide.hip) -> the symbol stage
//   OMP_ROUTE_WIDE   always the three-launch form with omp_wide_kernel
// A shape the chosen kernel cannot serve is an argument error before anything is launched, never a fallback: chain_route_choose
// (chain_route.hpp) decides, omp_stage_run (chain_fast_core.hpp) launches what it chose at the three call sites of the receiver;
// the MMSE modes have no OMP stage and ignore the route.
#include "rx_plan.hpp"

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
