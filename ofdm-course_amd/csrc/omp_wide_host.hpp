// Host side of the wide OMP route (ofdm_omp_wide.hip): its LDS layout, the shapes it serves and the choice between it and
// omp_batch_kernel.  Plain C++ with no device or runtime dependency, so that a stand-alone program can run it under the host
// sanitizers (tests/omp_wide_host_main.cpp).
#pragma once

namespace ofdm {

constexpr unsigned OMP_STAGE_LDS_LIMIT = 150 * 1024;     // the bound every stage of the Task-5 receiver refuses above
constexpr int OMP_WIDE_XFORM = 2048;                     // one 256-thread workgroup = one 2048-point transform (fft_core.hpp)
constexpr int OMP_WIDE_MAXT = 32;                        // FAST_MAXT: the picks of a pursuit live in the lanes of a wavefront

enum { OMP_ROUTE_AUTO = 0, OMP_ROUTE_BATCH = 1, OMP_ROUTE_WIDE = 2 };

struct OmpWideLayout {      // byte offsets into dynamic LDS
  unsigned off_fft, off_state, state_bytes, total;
};

// Transform scratch of the c0 stage (fft_lds_elems(2048) elements) and, once c0 sits in registers, on the same bytes the R = L^-1
// state of the refit, one copy per wavefront ([taps][taps | 1], omp_wave_rs): the four wavefronts of the workgroup run the
// refit of the one realisation redundantly, so that no pick, coefficient or stop decision crosses a barrier.
inline OmpWideLayout omp_wide_layout(int taps, bool f64) {
  const unsigned cs = f64 ? 16u : 8u;
  OmpWideLayout o;
  const unsigned fft_bytes = (cs * (unsigned)(OMP_WIDE_XFORM + (OMP_WIDE_XFORM >> 3) + 8) + 15u) & ~15u;
  o.state_bytes = (cs * (unsigned)taps * (unsigned)(taps | 1) + 15u) & ~15u;
  o.off_fft = 0;
  o.off_state = 0;
  o.total = 4 * o.state_bytes > fft_bytes ? 4 * o.state_bytes : fft_bytes;
  return o;
}

// nullptr when omp_wide_kernel serves the shape, else the reason
inline const char* omp_wide_refusal(int nfft, int k_atoms, int taps) {
  if (nfft == 8192) return "the wide OMP route is not built for Nfft 8192 (512, 1024, 2048, 4096)";
  if (!(nfft == 512 || nfft == 1024 || nfft == 2048 || nfft == 4096)) return "the wide OMP route needs Nfft 512, 1024, 2048 or 4096";
  if (k_atoms < 1 || k_atoms > nfft) return "the wide OMP route needs 1 <= K <= Nfft";
  if (taps < 1 || taps > OMP_WIDE_MAXT || taps > k_atoms) return "the wide OMP route needs 1 <= taps <= 32, taps <= K";
  return nullptr;
}

// route: what the caller asked for; batch_lds: omp_layout(...).total of omp_batch_kernel for the shape.  Returns OMP_ROUTE_BATCH or
// OMP_ROUTE_WIDE, or 0 with *why set: a route that cannot serve the shape is an error, never a fallback.
inline int omp_route_choose(int route, unsigned batch_lds, int nfft, int k_atoms, int taps, const char** why) {
  *why = nullptr;
  const bool batch_ok = batch_lds <= OMP_STAGE_LDS_LIMIT;
  const char* wide_no = omp_wide_refusal(nfft, k_atoms, taps);
  switch (route) {
    case OMP_ROUTE_AUTO:
      if (batch_ok) return OMP_ROUTE_BATCH;
      if (!wide_no) return OMP_ROUTE_WIDE;
      *why = wide_no;
      return 0;
    case OMP_ROUTE_BATCH:
      if (batch_ok) return OMP_ROUTE_BATCH;
      *why = "omp_batch_kernel's state does not fit the LDS at this shape (OMP stage needs more than 150 KB)";
      return 0;
    case OMP_ROUTE_WIDE:
      if (!wide_no) return OMP_ROUTE_WIDE;
      *why = wide_no;
      return 0;
  }
  *why = "route must be 0 (library's choice), 1 (omp_batch_kernel) or 2 (wide)";
  return 0;
}

}  // namespace ofdm
