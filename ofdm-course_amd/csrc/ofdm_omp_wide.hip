// OMP_estimate.m:7-23 for a DFT dictionary of K <= Nfft consecutive delays on ANY pilot set, one realisation per 256-thread
// workgroup: the route of the Task-5 part-2 tiles (ofdm_part2.hip) for dictionaries whose omp_batch_kernel state does not fit
// the LDS -- F = dftmtx(Nfft) with all columns on a random pilot mask (Task5_part2.m:58-64, :181-184), and the pilots-only
// frame of Main_model_Task_5.m in double.
//
//   c0 = S^H Y     never touches the dictionary: for atoms exp(-2 pi i (pilot_p - 1) k / Nfft) it is the Nfft-point transform
//                  of Y scattered onto its carriers, c0 = conj(FFT(conj(Y_scattered)))[0..K).  Nfft <= 2048: ONE 2048-point
//                  workgroup transform (wg_fft, fft_core.hpp) with carrier c at input 2048 / Nfft * c; Nfft = 4096: a radix-2
//                  decimation-in-frequency stage in registers, then two of them (even / odd atoms).  P.sct is not read.
//   scores         c0 stays in registers for the whole pursuit: 8 atoms per thread (16 at Nfft 4096).  Every iteration
//                  recomputes c = c0 - sum_q g(idx_q - k) x_q atom by atom in the order omp_frame_wave uses -- the refit moves
//                  EVERY coefficient, so an incremental update costs the same and would add its own rounding.  g is the plan's
//                  one-sided Gram table read from global memory (64 KB at K = 4096, consecutive in k, shared by every
//                  workgroup, L2-resident); the negative shifts are its conjugates.
//   arg-max        first maximum in index order (OMP_estimate.m:7, :14): ascending k inside a thread, DPP butterflies inside a
//                  wavefront (largest score, then smallest index), then the four wave partials through LDS, lowest k winning
//                  equal scores at both levels.  The winner's c0 value travels with its partial: it is b_n of the refit.
//   refit          omp_wave_refit (omp_wave_core.hpp), run by all four wavefronts redundantly on their own copy of R = L^-1:
//                  one barrier per iteration (the partials), none for the state.
// Picks and coefficients land in P.tap_idx / P.tap_x as omp_batch_kernel leaves them.
#include "omp_wave_core.hpp"
#include "omp_wide_host.hpp"

namespace ofdm {

static_assert(fft_lds_elems(OMP_WIDE_XFORM) == OMP_WIDE_XFORM + (OMP_WIDE_XFORM >> 3) + 8, "omp_wide_layout restates fft_lds_elems");
static_assert(omp_wave_rs(10) == (10 | 1) && OMP_WIDE_MAXT == FAST_MAXT, "omp_wide_layout restates omp_wave_rs / FAST_MAXT");

// NE atoms per thread: 8 = one 2048-point transform (atom of slot s: tid + 256 s), 16 = Nfft 4096 (atom 2 tid + 512 (s / 2) + s % 2)
template <int NE>
__device__ __forceinline__ int wide_atom(int tid, int s) {
  return NE == 8 ? tid + 256 * s : 2 * tid + 512 * (s >> 1) + (s & 1);
}

template <typename T, int NE>
__global__ __launch_bounds__(256) void omp_wide_kernel(FastParams<T> P, OmpWideLayout lay, int lg_up, int64_t n_frames,
                                                       const cx<T>* __restrict__ tw_m) {
  static_assert(NE == 8 || NE == 16, "one or two 2048-point transforms");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ float part_s[2][4];                 // wave partials of the arg-max, two iterations deep (one barrier per iteration)
  __shared__ int part_k[2][4];
  __shared__ cx<T> part_c[2][4];
  cx<T>* const fl = (cx<T>*)(smem + lay.off_fft);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  cx<T>* const Rm = (cx<T>*)(smem + lay.off_state + (size_t)wave * lay.state_bytes);
  const int np = P.np, K = P.k_atoms, taps = P.taps;
  const T g0 = (T)P.gram[0].x;
  // a_k^H a_{k+d}, d in (-K, K)
  const auto gram = [&](int d) {
    const c64 gq = P.gram[d >= 0 ? d : -d];
    return mk<T>((T)gq.x, (T)(d >= 0 ? gq.y : -gq.y));
  };
  for (int64_t f = blockIdx.x; f < n_frames; f += gridDim.x) {
    const cx<T>* __restrict__ Y = P.ypil + f * np;
    double ynorm = 0;                            // ||Y||^2, every wavefront for itself
    for (int p = lane; p < np; p += 64) ynorm += (double)Y[p].x * Y[p].x + (double)Y[p].y * Y[p].y;
    for (int off = 32; off > 0; off >>= 1) ynorm += __shfl_xor(ynorm, off, 64);
    // ---- c0 = S^H Y = conj(FFT(conj(Y scattered onto its carriers)))
    cx<T> c0r[NE];
    if constexpr (NE == 8) {
      cx<T> v[8];
      const int um = (1 << lg_up) - 1;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = tid + 256 * e;
        const int p = (i & um) == 0 ? (int)P.prole[i >> lg_up] : -1;
        v[e] = p >= 0 ? conj(Y[p]) : mk<T>(0, 0);
      }
      wg_fft<T, OMP_WIDE_XFORM, false>(v, tid, tw_m, fl);
#pragma unroll
      for (int e = 0; e < 8; ++e) c0r[e] = conj(v[e]);
    } else {
      // X[2 m] = FFT_2048(x[n] + x[n + 2048])[m],  X[2 m + 1] = FFT_2048((x[n] - x[n + 2048]) W_4096^n)[m]
      cx<T> a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int i = tid + 256 * e;
        const int p0 = P.prole[i], p1 = P.prole[i + 2048];
        const cx<T> x0 = p0 >= 0 ? conj(Y[p0]) : mk<T>(0, 0), x1 = p1 >= 0 ? conj(Y[p1]) : mk<T>(0, 0);
        a[e] = x0 + x1;
        b[e] = (x0 - x1) * P.tw[i];
      }
      wg_fft<T, OMP_WIDE_XFORM, false>(a, tid, tw_m, fl);
      wg_fft<T, OMP_WIDE_XFORM, false>(b, tid, tw_m, fl);          // (its first barrier follows the gathers of the call above)
#pragma unroll
      for (int e = 0; e < 8; ++e) { c0r[2 * e] = conj(a[e]); c0r[2 * e + 1] = conj(b[e]); }
    }
    __syncthreads();                             // the transform scratch is dead: the R states take the bytes
    OmpWaveState<T> s;
    omp_wave_begin<T>(s, Rm, taps, true, ynorm);
    for (int it = 0; it < taps && s.active; ++it) {                // (s.active and the break below are workgroup-uniform)
      const int ns = __builtin_amdgcn_readfirstlane(s.n);
      // ---- residual correlation c = c0 - G(:, index) x and its first arg-max (OMP_estimate.m:7,:14)
      float bs = -1.0f;
      int bi = 0x7fffffff;
      cx<T> bc = c0r[0];                         // c0 at the thread's best atom
#pragma unroll
      for (int h = 0; h < NE / 8; ++h) {
        cx<T> c[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) c[u] = c0r[8 * h + u];
        if (ns > 0) {
          cx<T> ga[8], gb[8];
          const int p0 = __builtin_amdgcn_readlane(s.pk, 0);
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int k = wide_atom<NE>(tid, 8 * h + u);
            ga[u] = k < K ? gram(p0 - k) : mk<T>(0, 0);
          }
          for (int q = 0; q < ns; ++q) {         // the next pick's Gram values are in flight
            const cx<T> xa = lane_bcast(s.xq, q);
            const int pn = __builtin_amdgcn_readlane(s.pk, q + 1 < ns ? q + 1 : q);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int k = wide_atom<NE>(tid, 8 * h + u);
              gb[u] = k < K ? gram(pn - k) : mk<T>(0, 0);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              if constexpr (sizeof(T) == 4) cmsub(c[u], ga[u], xa); else c[u] = c[u] - ga[u] * xa;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) ga[u] = gb[u];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int k = wide_atom<NE>(tid, 8 * h + u);
          if (k < K) {
            float sc;
            if constexpr (sizeof(T) == 4) sc = c[u].x * c[u].x + c[u].y * c[u].y;     // fp32 mode: near-ties fall under the 1e-4 rule
            else sc = (float)((double)c[u].x * c[u].x + (double)c[u].y * c[u].y);
            if (sc > bs) { bs = sc; bi = k; bc = c0r[8 * h + u]; }       // ascending k inside a thread: strict > keeps the first
          }
        }
      }
      const float gmax = group_max_f(bs, 64, lane);
      const int wb = group_min_i(bs == gmax ? bi : 0x7fffffff, 64, lane);
      const unsigned long long own = __ballot(bs == gmax && bi == wb);
      if (lane == (own ? __builtin_ctzll(own) : 0)) {
        part_s[it & 1][wave] = gmax; part_k[it & 1][wave] = wb; part_c[it & 1][wave] = bc;
      }
      __syncthreads();
      float ws = part_s[it & 1][0];
      int wk = part_k[it & 1][0];
      cx<T> bn = part_c[it & 1][0];
#pragma unroll
      for (int w = 1; w < 4; ++w) {              // wave order; the lowest k wins equal scores
        const float s2 = part_s[it & 1][w];
        const int k2 = part_k[it & 1][w];
        if (s2 > ws || (s2 == ws && k2 < wk)) { ws = s2; wk = k2; bn = part_c[it & 1][w]; }
      }
      const int kp = wk < K ? wk : 0;            // all-NaN scores: MATLAB max returns index 1 (thread 0 holds c0[0])
      if (!omp_wave_refit<T>(s, it, ns, kp, gram, [&]() { return bn; }, g0, Rm, taps)) break;
    }
    if (wave == 0) omp_wave_store<T>(P, s, taps, f);
    __syncthreads();                             // the R states and the partials are reused by the next realisation
  }
}

// omp_wide_kernel over n_frames realisations: pilot LS values P.ypil -> taps P.tap_idx / P.tap_x.  P.tw: the Nfft table.
template <typename T>
int omp_wide_run(const FastParams<T>& P, int nfft, int64_t n_frames) {
  const char* why = omp_wide_refusal(nfft, P.k_atoms, P.taps);
  OFDM_ARG(!why, "OMP_estimate: %s", why);
  const OmpWideLayout lay = omp_wide_layout(P.taps, sizeof(T) == 8);
  OFDM_ARG(lay.total <= OMP_STAGE_LDS_LIMIT, "OMP_estimate: the wide OMP stage needs %u bytes of LDS", lay.total);
  if (n_frames <= 0) return OFDM_OK;
  hipStream_t st = ctx().stream;
  const void* twm = nullptr;
  OFDM_TRY(get_twiddles(OMP_WIDE_XFORM, std::is_same<T, double>::value, &twm));
  int lg_up = 0;
  while (nfft < OMP_WIDE_XFORM && (nfft << lg_up) < OMP_WIDE_XFORM) ++lg_up;
  auto launch = [&](auto kern) -> int {
    // (set on every call: the attribute belongs to the device the context is on now)
    OFDM_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lay.total));
    const int per_cu = resident_blocks_per_cu((const void*)kern, 256, lay.total);
    const unsigned grid = (unsigned)std::min<int64_t>(n_frames, (int64_t)ctx().num_cu * std::max(1, per_cu));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lay.total, st, P, lay, lg_up, n_frames, (const cx<T>*)twm);
    return OFDM_OK;
  };
  if (nfft == 4096) OFDM_TRY(launch(omp_wide_kernel<T, 16>));
  else OFDM_TRY(launch(omp_wide_kernel<T, 8>));
  return check_launch("omp_wide_kernel");
}
template int omp_wide_run<float>(const FastParams<float>&, int, int64_t);
template int omp_wide_run<double>(const FastParams<double>&, int, int64_t);

}  // namespace ofdm
