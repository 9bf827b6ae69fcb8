// Stand-alone driver of the host side of the wide OMP route (csrc/omp_wide_host.hpp: LDS layout, supported shapes, route choice)
// for tests/test_omp_wide_inputs_host.py, which builds it with the address and undefined-behaviour sanitizers.
//   omp_wide_host_main sweep            every required (Nfft, K, taps, precision): layout within the LDS bound, shape accepted,
//                                       the route choice for a batch state below / at / above the bound; prints one line per
//                                       (taps, precision) with the layout, then the number of shapes visited
//   omp_wide_host_main choose ROUTE BATCH_LDS NFFT K TAPS     prints the chosen route (1 / 2), or 0 and the reason
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ofdm-course_amd/csrc/omp_wide_host.hpp"

using namespace ofdm;

static int fail(const char* what, int nfft, int k, int taps, int f64) {
  std::fprintf(stderr, "FAILED: %s at Nfft %d K %d taps %d f64 %d\n", what, nfft, k, taps, f64);
  return 1;
}

int main(int argc, char** argv) {
  if (argc == 7 && !std::strcmp(argv[1], "choose")) {
    const char* why = nullptr;
    const int r = omp_route_choose(std::atoi(argv[2]), (unsigned)std::strtoul(argv[3], nullptr, 10), std::atoi(argv[4]),
                                   std::atoi(argv[5]), std::atoi(argv[6]), &why);
    std::printf("%d %s\n", r, why ? why : "-");
    return 0;
  }
  if (argc != 2 || std::strcmp(argv[1], "sweep")) return 2;
  long visited = 0;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int taps = 1; taps <= OMP_WIDE_MAXT; ++taps) {
      const OmpWideLayout lay = omp_wide_layout(taps, f64 != 0);
      std::printf("layout f64 %d taps %d state %u total %u\n", f64, taps, lay.state_bytes, lay.total);
      if (lay.total > OMP_STAGE_LDS_LIMIT || lay.off_state + 4 * lay.state_bytes > lay.total || (lay.state_bytes & 15u))
        return fail("layout", 0, 0, taps, f64);
      for (int nfft = 512; nfft <= 4096; nfft *= 2)
        for (int k = taps; k <= nfft; ++k) {
          const char* why = nullptr;
          if (omp_wide_refusal(nfft, k, taps)) return fail("refused a required shape", nfft, k, taps, f64);
          if (omp_route_choose(OMP_ROUTE_AUTO, OMP_STAGE_LDS_LIMIT, nfft, k, taps, &why) != OMP_ROUTE_BATCH || why)
            return fail("auto at the bound", nfft, k, taps, f64);
          if (omp_route_choose(OMP_ROUTE_AUTO, OMP_STAGE_LDS_LIMIT + 1, nfft, k, taps, &why) != OMP_ROUTE_WIDE || why)
            return fail("auto above the bound", nfft, k, taps, f64);
          if (omp_route_choose(OMP_ROUTE_BATCH, OMP_STAGE_LDS_LIMIT + 1, nfft, k, taps, &why) != 0 || !why)
            return fail("forced batch above the bound", nfft, k, taps, f64);
          if (omp_route_choose(OMP_ROUTE_WIDE, 0, nfft, k, taps, &why) != OMP_ROUTE_WIDE || why)
            return fail("forced wide", nfft, k, taps, f64);
          ++visited;
        }
    }
  // outside the required set: every one is a refusal with a reason, on the forced and on the automatic route
  const int bad[][3] = {{8192, 4096, 7}, {256, 256, 7}, {1000, 512, 7}, {4096, 4097, 7}, {4096, 0, 1}, {4096, 4096, 33}, {512, 4, 5}};
  for (const auto& b : bad) {
    const char* why = nullptr;
    if (!omp_wide_refusal(b[0], b[1], b[2])) return fail("accepted an unsupported shape", b[0], b[1], b[2], 0);
    if (omp_route_choose(OMP_ROUTE_WIDE, 0, b[0], b[1], b[2], &why) != 0 || !why) return fail("forced wide, unsupported", b[0], b[1], b[2], 0);
    if (omp_route_choose(OMP_ROUTE_AUTO, OMP_STAGE_LDS_LIMIT + 1, b[0], b[1], b[2], &why) != 0 || !why)
      return fail("auto, unsupported", b[0], b[1], b[2], 0);
    if (omp_route_choose(OMP_ROUTE_AUTO, 1024, b[0], b[1], b[2], &why) != OMP_ROUTE_BATCH) return fail("auto keeps batch", b[0], b[1], b[2], 0);
  }
  const char* why = nullptr;
  if (omp_route_choose(3, 0, 512, 512, 7, &why) != 0 || !why) return fail("route 3", 512, 512, 7, 0);
  std::printf("visited %ld\n", visited);
  return 0;
}
