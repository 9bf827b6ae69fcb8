// Constellation capture of the Task-4 receiver and sweep (ofdm_rx_chain_task4_iq, ofdm_ber_sweep_task4_scope) and of the Task-5
// ones (ofdm_rx_chain_task5_iq, ofdm_ber_sweep_task5_scope; the scope5_* functions): the argument checks of the entries in the
// order they are made, the LDS the density grid adds to a symbol stage's (eq_demap_kernel's for Task 4, ofdm_chain_split.hip)
// and the bin of a value -- decided before anything is launched or allocated.  Plain C++ with no device or runtime dependency:
// tests/host/scope_plan_main.cpp runs it under the host sanitizers against the hand-written model of tests/scope_cases.py.
// scope_bin is the one function that bins, on the device (eq_demap_kernel) and on the host: OFDM_SCOPE_HD is the device
// qualifier where the device compiler reads this file and empty elsewhere.  The .hip side turns a refusal into OFDM_ERR_ARG with
// ScopeWhy::text as the last-error string.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "chain_route.hpp"      // STAGE_LDS_LIMIT, eq_demap_lds_bytes

#if defined(__HIPCC__)
#define OFDM_SCOPE_HD __host__ __device__
#else
#define OFDM_SCOPE_HD
#endif

namespace ofdm {

enum { SCOPE_OK = 0, SCOPE_REFUSE_IQ_FIRST, SCOPE_REFUSE_IQ_COUNT, SCOPE_REFUSE_IQ_END, SCOPE_REFUSE_DENSITY_OUT, SCOPE_REFUSE_BINS,
       SCOPE_REFUSE_HALF_WIDTH, SCOPE_REFUSE_SKIP, SCOPE_REFUSE_LDS, SCOPE_REFUSALS };

struct ScopeWhy {
  char text[256] = "";
};

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline int scope_refuse(ScopeWhy& w, int id, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(w.text, sizeof(w.text), fmt, ap);
  va_end(ap);
  return id;
}

// ---- ofdm_rx_chain_task4_iq, made behind the checks of ofdm_rx_chain_task4_ex that need no device (plan, data carriers,
// mer_skip) and only when iq_out is given: iq_first >= 0 -> iq_count >= 1 -> the window ends at or before decisions = nd * N_symb
// (compared without forming iq_first + iq_count, which may not fit 64 bits)
inline int scope_iq_check(int64_t iq_first, int64_t iq_count, int64_t decisions, ScopeWhy& w) {
  if (!(iq_first >= 0)) return scope_refuse(w, SCOPE_REFUSE_IQ_FIRST, "rx_chain_task4_iq: iq_first must be >= 0 (%lld)", (long long)iq_first);
  if (!(iq_count >= 1)) return scope_refuse(w, SCOPE_REFUSE_IQ_COUNT, "rx_chain_task4_iq: iq_count must be >= 1 (%lld)", (long long)iq_count);
  if (iq_count > decisions - iq_first)
    return scope_refuse(w, SCOPE_REFUSE_IQ_END, "rx_chain_task4_iq: iq_first + iq_count must not exceed nd * N_symb = %lld", (long long)decisions);
  return SCOPE_OK;
}

// ---- the density grid: bins x bins uint32 in eq_demap_kernel's dynamic LDS, behind the stage's present regions
inline bool scope_bins_ok(int bins) { return bins == 8 || bins == 16 || bins == 32 || bins == 64 || bins == 128; }
inline size_t scope_grid_offset(bool f64, int n_carrier, int64_t decisions) {       // 16-byte aligned
  return route_align16(eq_demap_lds_bytes(f64, n_carrier, decisions));
}
inline size_t scope_grid_bytes(int bins) { return sizeof(uint32_t) * (size_t)bins * (size_t)bins; }
// what the grid adds to eq_demap_lds_bytes (the alignment padding included), and the stage's total with it
inline size_t scope_lds_extra(bool f64, int n_carrier, int64_t decisions, int bins) {
  return scope_grid_offset(f64, n_carrier, decisions) + scope_grid_bytes(bins) - eq_demap_lds_bytes(f64, n_carrier, decisions);
}
inline size_t scope_stage_lds(bool f64, int n_carrier, int64_t decisions, int bins) {
  return scope_grid_offset(f64, n_carrier, decisions) + scope_grid_bytes(bins);
}

// ---- ofdm_ber_sweep_task4_scope, made behind every check of ofdm_ber_sweep_task4_nmse (txf_task4_prelude, txf_plan.hpp):
// density_out -> bins -> half_width -> scope_skip 0 .. decisions - 1 -> the stage's LDS with the grid within STAGE_LDS_LIMIT
inline int scope_density_check(bool density_out, int bins, double half_width, int64_t scope_skip, bool f64, int n_carrier,
                               int64_t decisions, ScopeWhy& w) {
  if (!density_out)
    return scope_refuse(w, SCOPE_REFUSE_DENSITY_OUT, "ber_sweep_task4_scope: density_out missing (ofdm_ber_sweep_task4_nmse is the call without it)");
  if (!scope_bins_ok(bins)) return scope_refuse(w, SCOPE_REFUSE_BINS, "ber_sweep_task4_scope: bins must be 8, 16, 32, 64 or 128 (%d)", bins);
  if (!(std::isfinite(half_width) && half_width > 0.0))
    return scope_refuse(w, SCOPE_REFUSE_HALF_WIDTH, "ber_sweep_task4_scope: half_width must be finite and > 0");
  if (!(scope_skip >= 0 && scope_skip < decisions))
    return scope_refuse(w, SCOPE_REFUSE_SKIP, "ber_sweep_task4_scope: scope_skip must be 0 .. nd * N_symb - 1 (%lld)", (long long)scope_skip);
  const size_t lds = scope_stage_lds(f64, n_carrier, decisions, bins);
  if (lds > STAGE_LDS_LIMIT)
    return scope_refuse(w, SCOPE_REFUSE_LDS, "ber_sweep_task4_scope: the equalise / demap stage with a %d x %d grid needs %zu bytes of LDS (at most %zu)",
                        bins, bins, lds, (size_t)STAGE_LDS_LIMIT);
  return SCOPE_OK;
}

// ---- the Task-5 receiver and sweeps (ofdm_rx_chain_task5_iq, ofdm_ber_sweep_task5_scope).  A capture call takes the route of
// the same call with the MER sums wanted (chain_route.hpp); every symbol stage of that route has a Scope variant that keeps the
// grid in dynamic LDS behind the stage's own regions, 16-byte aligned.
// ofdm_rx_chain_task5_iq: the three refusals of scope_iq_check, behind the checks and the route of ofdm_rx_chain_task5_ex
inline int scope5_iq_check(int64_t iq_first, int64_t iq_count, int64_t decisions, ScopeWhy& w) {
  if (!(iq_first >= 0)) return scope_refuse(w, SCOPE_REFUSE_IQ_FIRST, "rx_chain_task5_iq: iq_first must be >= 0 (%lld)", (long long)iq_first);
  if (!(iq_count >= 1)) return scope_refuse(w, SCOPE_REFUSE_IQ_COUNT, "rx_chain_task5_iq: iq_count must be >= 1 (%lld)", (long long)iq_count);
  if (iq_count > decisions - iq_first)
    return scope_refuse(w, SCOPE_REFUSE_IQ_END, "rx_chain_task5_iq: iq_first + iq_count must not exceed nd * N_symb = %lld", (long long)decisions);
  return SCOPE_OK;
}

// the dynamic LDS of the symbol stage a route names, without a grid (the wave stage's is its layout's: four wavefronts per workgroup)
inline size_t scope5_stage_lds(const ChainRoute& r, int nd, int n_symb) {
  if (r.symbols == SYM_GENERIC) return r.generic_lds;
  if (r.symbols == SYM_WAVE) {
    WaveLayout wl{};
    (void)wave_layout(nd, n_symb, 4, wl);
    return wl.total;
  }
  return r.symbol_lds;
}
inline size_t scope5_grid_offset(size_t stage_lds_bytes) { return route_align16(stage_lds_bytes); }
// the stage's dynamic LDS of a call: with the grid behind its regions when a density is taken (bins != 0)
inline size_t scope5_lds_total(size_t stage_lds_bytes, int bins) {
  return bins ? scope5_grid_offset(stage_lds_bytes) + scope_grid_bytes(bins) : stage_lds_bytes;
}
inline size_t scope5_lds_limit(int stage) { return stage == SYM_GENERIC ? GENERIC_LDS_LIMIT : STAGE_LDS_LIMIT; }
inline const char* scope5_stage_name(int stage) {
  static const char* const NAMES[] = {"generic", "rx_symbols", "wave", "coop4", "r2", "eq_demap"};
  return stage >= SYM_GENERIC && stage <= SYM_EQ_DEMAP ? NAMES[stage] : "?";
}

// ofdm_ber_sweep_task5_scope, made behind every check of ofdm_ber_sweep_task5_fading / _ex (txf_task5_prelude, txf_plan.hpp):
// density_out -> bins -> half_width -> scope_skip 0 .. decisions - 1 -> the chosen symbol stage's LDS (stage = SYM_*,
// stage_lds_bytes = scope5_stage_lds) with the grid within that stage's limit
inline int scope5_density_check(int stage, size_t stage_lds_bytes, int bins, double half_width, int64_t scope_skip, int64_t decisions,
                                bool density_out, ScopeWhy& w) {
  if (!density_out)
    return scope_refuse(w, SCOPE_REFUSE_DENSITY_OUT, "ber_sweep_task5_scope: density_out missing (ofdm_ber_sweep_task5_fading / _ex are the calls without it)");
  if (!scope_bins_ok(bins)) return scope_refuse(w, SCOPE_REFUSE_BINS, "ber_sweep_task5_scope: bins must be 8, 16, 32, 64 or 128 (%d)", bins);
  if (!(std::isfinite(half_width) && half_width > 0.0))
    return scope_refuse(w, SCOPE_REFUSE_HALF_WIDTH, "ber_sweep_task5_scope: half_width must be finite and > 0");
  if (!(scope_skip >= 0 && scope_skip < decisions))
    return scope_refuse(w, SCOPE_REFUSE_SKIP, "ber_sweep_task5_scope: scope_skip must be 0 .. nd * N_symb - 1 (%lld)", (long long)scope_skip);
  const size_t lds = scope5_lds_total(stage_lds_bytes, bins);
  if (lds > scope5_lds_limit(stage))
    return scope_refuse(w, SCOPE_REFUSE_LDS, "ber_sweep_task5_scope: the %s symbol stage with a %d x %d grid needs %zu bytes of LDS (at most %zu)",
                        scope5_stage_name(stage), bins, bins, lds, scope5_lds_limit(stage));
  return SCOPE_OK;
}

// scale = bins / (2 * half_width), once per call on the host, in double
inline double scope_scale(int bins, double half_width) { return (double)bins / (2.0 * half_width); }

// The bin of one coordinate v (re for the column, im for the row), double arithmetic in both precisions:
//   clamp((int)floor((v + half_width) * scale), 0, bins - 1),   -1 for a non-finite v (the point is dropped, not binned).
// The clamp is made on the floor before it is converted, so that a finite v far outside the grid (whose product does not fit
// an int, or is infinite) lands in the edge bin like any other.
OFDM_SCOPE_HD inline int scope_bin(double v, double half_width, double scale, int bins) {
  if (!(v - v == 0.0)) return -1;                       // +-inf, NaN
  const double t = floor((v + half_width) * scale);
  if (!(t >= 0.0)) return 0;
  if (t >= (double)bins) return bins - 1;
  return (int)t;
}

}  // namespace ofdm
