// The batched Task-4 receiver (ofdm_rx_chain_task4, T4/Main_model_Task_4.m:278-347): its kernels, its stages and task4_run,
// which runs the stages the route of t4_route.hpp names.
#include <algorithm>

#include "scope_plan.hpp"
#include "spline_op.hpp"
#include "sync_core.hpp"
#include "t4_route.hpp"
#include "t4_stream.hpp"

namespace ofdm {

static_assert(ACF_MAXW == T4_ACF_MAXW, "t4_route_choose refuses guards beyond the autocorrelation's window limit");

int demod_device(const void* y, void* x, int nfft, int64_t n_symb, int t_guard, bool f64);   // ofdm_modem.hip

// ---------------------------------------------------------------------------------------------
// Batched receiver (ofdm_rx_chain_task4): AutoCorrFunction.m:3-24 for one frame per workgroup WITHOUT the curve -- the
// receiver needs TgPosition and AutoCorr(TgPosition) only (T4/Main_model_Task_4.m:278-303).  The tiles of acf_tile are
// walked in order (so every rho value is bit-identical to acf_kernel's), each tile's rho stays in LDS, and the search of
// :10-20 -- first index > WidthWindow above the threshold (f), first one below after it (g), first one above after that
// (h: a second run exists) -- advances through the tile as a three-state machine; the walk stops at h (a symbol and a
// half into the frame on average) or at the end of the stream (the catch branch, TgPosition = 65).  Replaces five
// launches (rho of a three-symbol prefix -> plateau search -> list of unresolved frames -> rho of those over the whole
// stream -> search again -> per-frame scalars) and the 0.5 GB round trip of the prefix curve.
//   tg[f] = TgPosition, fo[f] = -angle(AutoCorr(TgPosition)) / (2 pi)  (:27), status[f] = 0 / 1 (catch branch) / -2 (index error at :27)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(ACF_THREADS) void t4_acf_search_kernel(const cx<T>* __restrict__ x_all, int64_t len, int W, int nfft,
                                                                    int64_t n_out, double thr, int64_t* __restrict__ tg,
                                                                    double* __restrict__ fo, int32_t* __restrict__ status) {
  using acc = acf4<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char acf_smem[];
  acc* const S = (acc*)acf_smem;
  cx<T>* const rt = (cx<T>*)(S + ACF_TILE + W + 1);  // rho of the current tile
  __shared__ acc wtot[ACF_THREADS / 64];
  __shared__ int wmin[ACF_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t fr = blockIdx.x;
  const cx<T>* const x = x_all + fr * len;
  auto tile = [&](int64_t n0) {
    const int n_here = (int)((n_out - n0 < ACF_TILE) ? (n_out - n0) : ACF_TILE);
    acf_tile<T>(x, n0, n_here, W, nfft, S, wtot, [rt](int i, cx<T> r) { rt[i] = r; });
    __syncthreads();
    return n_here;
  };
  // the smallest i in [lo, n_here) of the tile in LDS whose |rho| is above (want_above) / not above the threshold, or -1
  auto first_in_tile = [&](int lo, int n_here, bool want_above) -> int {
    int best = 0x7fffffff;
    for (int i = lo + tid; i < n_here; i += ACF_THREADS) {        // ascending per thread: its first hit is its smallest
      const cx<T> v = rt[i];
      const bool ab = sqrt((double)v.x * v.x + (double)v.y * v.y) > thr;
      if (ab == want_above) { best = i; break; }
    }
    for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
    if (lane == 0) wmin[wid] = best;
    __syncthreads();
    int r = wmin[0];
    for (int w = 1; w < ACF_THREADS / 64; ++w) r = min(r, wmin[w]);
    __syncthreads();
    return r == 0x7fffffff ? -1 : r;
  };
  int stage = 0;                                      // 0: looking for f, 1: g, 2: h, 3: found
  int64_t from = W, f0 = -1, g0 = -1;                 // 1-based index idx = i + 1 must be > W  <=>  i >= W
  int64_t cur_n0 = -1;
  for (int64_t n0 = (from / ACF_TILE) * ACF_TILE; n0 < n_out && stage < 3; n0 += ACF_TILE) {
    const int n_here = tile(n0);
    cur_n0 = n0;
    while (stage < 3) {
      const int lo = from > n0 ? (int)(from - n0) : 0;
      const int r = lo < n_here ? first_in_tile(lo, n_here, stage != 1) : -1;
      if (r < 0) break;
      if (stage == 0) f0 = n0 + r; else if (stage == 1) g0 = n0 + r;
      from = n0 + r + 1;
      ++stage;
    }
  }
  const int ok = stage == 3;
  const int64_t pos = ok ? ((f0 + 1) + (g0 - 1 + 1)) / 2 : 65;   // :20 floor of the mean of the run's 1-based ends; :23
  double vr = NAN, vi = NAN;
  if (pos >= 1 && pos <= n_out) {
    const int64_t pn0 = ((pos - 1) / ACF_TILE) * ACF_TILE;
    if (pn0 != cur_n0) tile(pn0);                    // the plateau's tile is no longer (or was never) the one in LDS
    const cx<T> v = rt[pos - 1 - pn0];
    vr = (double)v.x; vi = (double)v.y;
  }
  if (tid == 0) {
    tg[fr] = pos;
    fo[fr] = -atan2(vi, vr) / (2.0 * M_PI);
    status[fr] = pos > n_out ? -2 : (ok ? 0 : 1);
  }
}

template <typename T> inline size_t acf_search_lds_bytes(int W) { return acf_lds_bytes<T>(W) + sizeof(cx<T>) * ACF_TILE; }


// ---------------------------------------------------------------------------------------------
// Task-4 receiver for a batch of frames (ofdm_rx_chain_task4): every stage above with grid.x / grid.y = frame, the
// per-frame scalars (TgPosition, FreqOffset, IFO, fine-sync estimates) never leave the device.
// ---------------------------------------------------------------------------------------------
// plateau result -> TgPosition, FreqOffset = -angle(rho(TgPosition)) / (2 pi) (AutoCorrFunction.m:27), status
__global__ void t4_scalars_kernel(const int64_t* __restrict__ res, const double* __restrict__ resv, int64_t n_out,
                                  int64_t* __restrict__ tg, double* __restrict__ fo, int32_t* __restrict__ status,
                                  int64_t n_frames) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  const int64_t pos = res[2 * f];
  tg[f] = pos;
  fo[f] = -atan2(resv[2 * f + 1], resv[2 * f]) / (2.0 * M_PI);
  status[f] = pos > n_out ? -2 : (res[2 * f + 1] ? 0 : 1);     // -2: index error at :27, 1: catch branch (65)
}

// add_STO(rx, TgPosition), add_STO(., -(Nfft+Tg)) (T4/Main_model_Task_4.m:292-294) and add_CFO(., -FreqOffset) (:301) in
// one pass: the shifts are copies, the rotation is the arithmetic of cfo_kernel.
template <typename T>
__global__ void t4_align_kernel(const cx<T>* __restrict__ rx, cx<T>* __restrict__ y, int64_t len, int sym_len, int nfft,
                                int time_desync, int freq_desync, const int64_t* __restrict__ tg,
                                const double* __restrict__ fo) {
  const int64_t f = blockIdx.y;
  const cx<T>* x = rx + f * len;
  cx<T>* o = y + f * len;
  const int64_t pos = time_desync ? tg[f] : 0;
  const double cfo = freq_desync ? -fo[f] : 0.0;
  const double inv_nfft = 1.0 / (double)nfft;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    cx<T> v = mk<T>(0, 0);
    if (time_desync) {
      const int64_t i1 = i - sym_len;                              // index in add_STO(rx, pos)
      if (i1 >= 0 && i1 < len - pos && i1 + pos < len) v = x[i1 + pos];
    } else {
      v = x[i];
    }
    if (freq_desync) {
      const double t = cfo * (double)i * inv_nfft;
      const double fr = t - floor(t);
      double sn, cs;
      sincospi(2.0 * fr, &sn, &cs);
      v = mk<T>((T)((double)v.x * cs - (double)v.y * sn), (T)((double)v.x * sn + (double)v.y * cs));
    }
    o[i] = v;
  }
}

// rx_signal(Nfft+1 : 2*Nfft) of every frame, contiguous (remove_IFO.m:5)
template <typename T>
__global__ void t4_segment_kernel(const cx<T>* __restrict__ y, cx<T>* __restrict__ seg, int64_t len, int nfft) {
  const int64_t f = blockIdx.y;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nfft; k += gridDim.x * blockDim.x)
    seg[f * nfft + k] = y[f * len + nfft + k];
}

// add_CFO(., -IFO) in place (remove_IFO.m:9); frames without a line above 0.77 are marked (MATLAB would abort)
template <typename T>
__global__ void t4_ifo_kernel(cx<T>* __restrict__ y, int64_t len, int nfft, const int64_t* __restrict__ first,
                              int32_t* __restrict__ ifo_out, int32_t* __restrict__ status) {
  const int64_t f = blockIdx.y;
  const int64_t fi = first[f];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ifo_out[f] = (int32_t)fi;
    if (fi < 0 && status[f] >= 0) status[f] = -1;
  }
  if (fi <= 0) return;                                             // nothing to rotate
  const double cfo = -(double)fi, inv_nfft = 1.0 / (double)nfft;
  cx<T>* o = y + f * len;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
    const double t = cfo * (double)i * inv_nfft;
    const double fr = t - floor(t);
    double sn, cs;
    sincospi(2.0 * fr, &sn, &cs);
    const cx<T> v = o[i];
    o[i] = mk<T>((T)((double)v.x * cs - (double)v.y * sn), (T)((double)v.x * sn + (double)v.y * cs));
  }
}

// ---- the same three stages without the intermediate streams (Nfft 512..4096): sample i of the aligned, CFO- and
// IFO-corrected stream of a frame, computed from rx on the fly with the roundings of the separate stages
// (round to T after the add_CFO(-FreqOffset) rotation and again after the add_CFO(-IFO) rotation).
// t4_raw / t4_rotate: t4_stream.hpp.

// rx_signal(Nfft+1 : 2*Nfft) after the STO fix and add_CFO(-FreqOffset), straight from rx (remove_IFO.m:5)
template <typename T>
__global__ void t4_segment_direct_kernel(const cx<T>* __restrict__ rx, cx<T>* __restrict__ seg, int64_t len, int sym_len, int nfft,
                                         int time_desync, const int64_t* __restrict__ tg, const double* __restrict__ fo) {
  const int64_t f = blockIdx.y;
  const int64_t pos = time_desync ? tg[f] : 0;
  const double cfo = -fo[f], inv = 1.0 / (double)nfft;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nfft; k += gridDim.x * blockDim.x) {
    const int64_t i = (int64_t)nfft + k;
    seg[f * nfft + k] = t4_rotate<T>(t4_raw<T>(rx + f * len, i, len, sym_len, time_desync, pos), cfo, i, inv);
  }
}

__global__ void t4_ifo_finalize_kernel(const int64_t* __restrict__ first, int32_t* __restrict__ ifo_out,
                                       int32_t* __restrict__ status, int64_t n_frames) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  ifo_out[f] = (int32_t)first[f];
  if (first[f] < 0 && status[f] >= 0) status[f] = -1;
}

// OFDM_demodulator of every symbol of every frame on the wave-local transform, its samples taken from rx through
// t4_raw / t4_rotate: no aligned / corrected copy of the batch is ever written.
template <typename T, int NW>
__global__ __launch_bounds__(64 * NW) void t4_demod_kernel(const cx<T>* __restrict__ rx, cx<T>* __restrict__ X,
                                                           const cx<T>* __restrict__ tw, int64_t len, int t_guard, int n_symb,
                                                           int64_t n_frames, int time_desync, int freq_desync,
                                                           const int64_t* __restrict__ tg, const double* __restrict__ fo,
                                                           const int32_t* __restrict__ ifo, int n_keep,
                                                           cx<T>* __restrict__ xp, const int16_t* __restrict__ prole, int np) {
  constexpr int N = 512 * NW;
  constexpr int BPT = NW > 1 ? 8 / NW : 8;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  cx<T>* lwv = (cx<T>*)smem;
  cx<T>* const ex = lwv;
  cx<T>* twl = lwv + NW * WAVE_LDS_ELEMS;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, gid = threadIdx.x;
  DifTw<T, NW> dt;
  wave_tw_fill<T, NW>(twl, tw);
  dif_tw_init<T, NW>(dt, gid, tw);
  cx<T> twb[7];
#pragma unroll
  for (int t = 1; t < 8; ++t) twb[t - 1] = tw[(t * (lane & 7) * 8) * NW];
  __syncthreads();
  const int sym_len = N + t_guard;
  const double inv = 1.0 / (double)N;
  const int64_t total = n_frames * n_symb;
  // slot e of this thread <-> sample m_e of the symbol (the layout frame_load uses)
  auto slot_m = [&](int e) -> int {
    if constexpr (NW == 1) return lane + 64 * e;
    else return gid * BPT + (e / NW) + 512 * (e % NW);
  };
  auto load_raw = [&](cx<T> (&dst)[8], int64_t sg) {
    const int64_t f = sg / n_symb;
    const int sy = (int)(sg - f * n_symb);
    const int64_t pos = time_desync ? tg[f] : 0;
    const cx<T>* xf = rx + f * len;
#pragma unroll
    for (int e = 0; e < 8; ++e) dst[e] = t4_raw<T>(xf, (int64_t)sy * sym_len + t_guard + slot_m(e), len, sym_len, time_desync, pos);
  };
  // phase (in turns) of the merged rotation add_CFO(-FreqOffset) . add_CFO(-IFO) at stream index i: the fractional part in
  // double, the integer-offset part reduced exactly in integers (N is a power of two)
  auto turns_at = [&](double c1, int32_t fi, int64_t i) -> double {
    double t = c1 * (double)i * inv;
    t -= floor(t);
    if (fi > 0) {
      t -= (double)(((int64_t)fi * i) & (N - 1)) * inv;
      t += t < 0.0 ? 1.0 : 0.0;
    }
    return t;
  };
  cx<T> v[8], nx[8];
  if ((int64_t)blockIdx.x < total) load_raw(nx, blockIdx.x);
  for (int64_t sg = blockIdx.x; sg < total; sg += gridDim.x) {
    const int64_t f = sg / n_symb;
    const int sy = (int)(sg - f * n_symb);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = nx[e];
    if (sg + gridDim.x < total) load_raw(nx, sg + gridDim.x);
    if (freq_desync) {
      const double c1 = -fo[f];
      const int32_t fi = ifo[f];
      if constexpr (std::is_same<T, float>::value) {
        // throughput mode: ONE rotation per sample.  The rotor of the thread's first sample comes from a sine / cosine of the
        // exactly reduced phase; its other samples sit at fixed distances (e / NW) + 512 (e % NW), whose rotors are
        // frame constants (wave-uniform: a handful of scalar sine / cosine pairs per symbol): rotor_e = rotor_0 * step_e.
        // (Each sample used to pay two double multiplies, a floor, a 64-bit product and a sincospif of its own.)
        const int64_t i0 = (int64_t)sy * sym_len + t_guard + slot_m(0);
        auto rotor = [&](int64_t i) {
          float sn, cs;
          sincospif(2.0f * (float)turns_at(c1, fi, i), &sn, &cs);
          return mk<float>(cs, sn);
        };
        const cx<float> r0 = rotor(i0);
        // distances (e / NW) + 512 (e % NW) [or 64 e for one wavefront per symbol]: powers of two base steps
        constexpr int SA = NW > 1 ? 512 : 64, NA = NW > 1 ? NW : 8, NB = NW > 1 ? BPT : 1;
        cx<float> pa[NA];                                         // rotor(SA a)
        pa[0] = mk<float>(1.0f, 0.0f);
        if (NA > 1) pa[1] = rotor(SA);
#pragma unroll
        for (int a = 2; a < NA; ++a) pa[a] = pa[a - 1] * pa[1];
        cx<float> pb = r0;                                        // r0 * rotor(b)
        const cx<float> r1 = NB > 1 ? rotor(1) : mk<float>(1.0f, 0.0f);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
          for (int a = 0; a < NA; ++a) {
            const int e = NW > 1 ? b * NW + a : a;
            v[e] = v[e] * (a == 0 ? pb : pb * pa[a]);
          }
          pb = pb * r1;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int64_t i = (int64_t)sy * sym_len + t_guard + slot_m(e);
          v[e] = t4_rotate<T>(v[e], c1, i, inv);
          if (fi > 0) v[e] = t4_rotate<T>(v[e], -(double)fi, i, inv);
        }
      }
    }
    if constexpr (NW > 1) {
      dif_stage<T, NW>(v, dt);
      __syncthreads();
      dif_scatter<T, NW>(v, gid, ex);
      __syncthreads();
      dif_gather<T>(v, wave, lane, ex);
    } else {
      __syncthreads();
    }
    wave_fft512<T, false>(v, lane, twb, twl, lwv + wave * WAVE_LDS_ELEMS);
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 8; ++t) lwv[NW * (lane + 64 * t) + wave] = v[t];
    __syncthreads();
    // rows 1..n_keep of the column (everything downstream reads carriers 1..N_carrier only) + its pilot rows, compact
    cx<T>* dst = X + sg * (int64_t)n_keep;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int i = gid + 64 * NW * e;
      if (i < n_keep) {
        const cx<T> xv = lwv[i];
        nt_store(dst + i, xv);
        if (xp) {
          const int pr = prole[i];
          if (pr >= 0) xp[sg * (int64_t)np + pr] = xv;
        }
      }
    }
  }
}

template <typename T, int NW>
static int t4_demod_launch(const void* rx, void* X, const void* tw, int64_t len, int t_guard, int n_symb, int64_t F, int td, int fd,
                           const int64_t* tg, const double* fo, const int32_t* ifo, int n_keep, void* xp, const void* prole, int np) {
  const size_t dyn = sizeof(cx<T>) * ((size_t)NW * WAVE_LDS_ELEMS + WAVE_TW_ELEMS);
  auto kern = t4_demod_kernel<T, NW>;
  const int per_cu = resident_blocks_per_cu((const void*)kern, 64 * NW, dyn);
  const unsigned grid = (unsigned)std::min<int64_t>(F * n_symb, (int64_t)ctx().num_cu * per_cu);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NW), dyn, ctx().stream, (const cx<T>*)rx, (cx<T>*)X, (const cx<T>*)tw, len, t_guard,
                     n_symb, F, td, fd, tg, fo, ifo, n_keep, (cx<T>*)xp, (const int16_t*)prole, np);
  return check_launch("t4_demod_kernel");
}

// estimate_channel.m:6 per frame, then the spline operator of :8 restricted to rows 1..N_carrier (what equalize_signal reads)
template <typename T>
__global__ void t4_mean_pilots_kernel(const cx<T>* __restrict__ X, const cx<T>* __restrict__ tx, const int32_t* __restrict__ pc0,
                                      cx<T>* __restrict__ hp, int nfft, int np, int n_symb,
                                      const double* __restrict__ fine_est /* rotation not yet applied to X, or null */,
                                      int time_desync, int freq_desync, int compact /* X = X(pilotCarriers,:) [np x S] per frame */) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t f = blockIdx.y;
  if (p >= np) return;
  const cx<T>* rx = X + f * (int64_t)(compact ? np : nfft) * n_symb;
  double rc = 1.0, rs = 0.0;
  if (fine_est) {                                                  // the rotation of fine_apply_kernel for row pc0[p]
    const double tau = fine_est[2 * f], ph = fine_est[2 * f + 1];
    double psn = 0.0, pcs = 1.0, cs = 1.0, sn = 0.0;
    if (freq_desync) sincos(ph, &psn, &pcs);
    if (time_desync) {
      const double t = tau * (double)pc0[p];
      sincospi(2.0 * (t - floor(t)), &sn, &cs);
    }
    rc = cs * pcs - sn * psn;
    rs = sn * pcs + cs * psn;
  }
  double ar = 0, ai = 0;
  const int row = pc0[p];
  for (int s0 = 0; s0 < n_symb; s0 += 10) {                       // ten strided samples requested together
    cx<T> xs[10], ts[10];
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      const int s = s0 + u < n_symb ? s0 + u : n_symb - 1;
      xs[u] = compact ? rx[(int64_t)s * np + p] : rx[(int64_t)s * nfft + row];
      ts[u] = tx[s * np + p];
    }
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      if (s0 + u < n_symb) {
        cx<T> xv = xs[u];
        if (fine_est) xv = mk<T>((T)((double)xv.x * rc - (double)xv.y * rs), (T)((double)xv.x * rs + (double)xv.y * rc));
        const cx<T> q = cdiv(xv, ts[u]);
        ar += (double)q.x;
        ai += (double)q.y;
      }
    }
  }
  hp[f * np + p] = mk<T>((T)(ar / (double)n_symb), (T)(ai / (double)n_symb));
}

// fine_sync's two estimates (T4/fine_sync.m:10-20, :32-37) and the pilot means of estimate_channel.m:6 of one frame in ONE
// workgroup: the frame's pilot rows (compact, written by the demodulator) come from HBM once and from L2 after that, and the
// rotation of fine_sync.m:24-27 is formed once per pilot row instead of once per (row, symbol) -- they used to be three
// launches, each one sweep through HBM.  The arithmetic is the bodies of fine_tau_kernel /
// fine_phase_kernel / t4_mean_pilots_kernel unchanged.  sync == 0: only the means (no estimates, no rotation).
template <typename T>
__global__ __launch_bounds__(FS_THREADS) void t4_fine_est_kernel(const cx<T>* __restrict__ xp, const cx<T>* __restrict__ tx,
                                                                 const int32_t* __restrict__ pc0, int nfft, int np, int n_symb,
                                                                 double deltak, int sync, int time_desync, int freq_desync,
                                                                 int mp_desync, double* __restrict__ est, cx<T>* __restrict__ hp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fe_smem[];
  double2* const rot = (double2*)fe_smem;            // [np] rotation of fine_sync.m:24-27 per pilot row
  __shared__ FsScratch sc;
  const int64_t f = blockIdx.x;
  const int M = np * n_symb;
  // the frame's pilot rows [np x n_symb] stay where the demodulator wrote them: 48 KB per frame at the C3 geometry, read three
  // times by this workgroup -- from L2 after the first touch.  (Staging them in LDS was slower: 3 instead of 8 resident
  // workgroups per CU and flat loads in the shared reduction bodies, 0.45 against 0.35 ms per 4096 frames.)
  const cx<T>* const lp = xp + f * (int64_t)M;
  double tau = 0.0, ph = 0.0;
  if (sync) {
    PilotView<T> pv{lp, tx, pc0, nfft, np, (int64_t)M, 0, 1};
    tau = fine_tau_body<T>(pv, deltak, 1 /* T4 variant */, sc);
    if (time_desync) {
      for (int p = threadIdx.x; p < np; p += FS_THREADS) {
        double cs, sn;
        fine_rot<T>(tau, pc0[p], cs, sn);
        rot[p] = make_double2(cs, sn);
      }
      __syncthreads();
    }
    ph = fine_phase_body<T>(pv, time_desync, tau, sc, time_desync ? rot : nullptr);
    if (threadIdx.x == 0) { est[2 * f] = tau; est[2 * f + 1] = ph; }
  }
  if (!mp_desync) return;
  for (int p = threadIdx.x; p < np; p += FS_THREADS) {           // t4_mean_pilots_kernel for pilot p
    double rc = 1.0, rs = 0.0;
    if (sync) {
      double psn = 0.0, pcs = 1.0, cs = 1.0, sn = 0.0;
      if (freq_desync) sincos(ph, &psn, &pcs);
      if (time_desync) {
        const double t = tau * (double)pc0[p];
        sincospi(2.0 * (t - floor(t)), &sn, &cs);
      }
      rc = cs * pcs - sn * psn;
      rs = sn * pcs + cs * psn;
    }
    double ar = 0, ai = 0;
    for (int s0 = 0; s0 < n_symb; s0 += 10) {                     // ten strided samples requested together
      cx<T> xs[10], ts[10];
#pragma unroll
      for (int u = 0; u < 10; ++u) {
        const int s = s0 + u < n_symb ? s0 + u : n_symb - 1;
        xs[u] = lp[s * np + p];
        ts[u] = tx[s * np + p];
      }
#pragma unroll
      for (int u = 0; u < 10; ++u) {
        if (s0 + u < n_symb) {
          cx<T> xv = xs[u];
          if (sync) xv = mk<T>((T)((double)xv.x * rc - (double)xv.y * rs), (T)((double)xv.x * rs + (double)xv.y * rc));
          const cx<T> q = cdiv(xv, ts[u]);
          ar += (double)q.x;
          ai += (double)q.y;
        }
      }
    }
    hp[f * np + p] = mk<T>((T)(ar / (double)n_symb), (T)(ai / (double)n_symb));
  }
}

// H(1..N_carrier) = W * Hp for T4_FT frames per workgroup: a weight is read once and used for all of them (one frame per
// workgroup re-read the 429 KB operator from L2 for every frame: 70 us per 1024 frames); the pilot means are wave-uniform
// reads.  double accumulation: the not-a-knot weights alternate in sign.
constexpr int T4_FT = 8;
template <typename T>
__global__ __launch_bounds__(128) void t4_apply_operator_kernel(const T* __restrict__ W, const cx<T>* __restrict__ hp,
                                                                cx<T>* __restrict__ hout, int n_out, int n_in, int64_t n_frames) {
  extern __shared__ __attribute__((aligned(16))) unsigned char t4_smem[];
  cx<T>* hs = (cx<T>*)t4_smem;                                     // [n_in][T4_FT]: the tile's pilot means
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t f0 = (int64_t)blockIdx.y * T4_FT;
  for (int i = threadIdx.x; i < n_in * T4_FT; i += blockDim.x) {
    const int f = i / n_in, j = i - f * n_in;
    hs[j * T4_FT + f] = f0 + f < n_frames ? hp[(f0 + f) * n_in + j] : mk<T>(0, 0);
  }
  __syncthreads();
  if (m >= n_out) return;
  double ar[T4_FT], ai[T4_FT];
#pragma unroll
  for (int f = 0; f < T4_FT; ++f) ar[f] = ai[f] = 0.0;
  for (int j0 = 0; j0 < n_in; j0 += 8) {                           // eight weights of the column in flight
    T w[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) w[u] = j0 + u < n_in ? W[(size_t)(j0 + u) * n_out + m] : T(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (j0 + u < n_in) {
        const double wd = (double)w[u];
#pragma unroll
        for (int f = 0; f < T4_FT; ++f) {
          const cx<T> z = hs[(j0 + u) * T4_FT + f];
          ar[f] += wd * (double)z.x;
          ai[f] += wd * (double)z.y;
        }
      }
    }
  }
#pragma unroll
  for (int f = 0; f < T4_FT; ++f)
    if (f0 + f < n_frames) hout[(f0 + f) * n_out + m] = mk<T>((T)ar[f], (T)ai[f]);
}

__global__ void t4_init_kernel(int32_t* __restrict__ stat, int64_t* __restrict__ tg, double* __restrict__ fo, int32_t* __restrict__ ifo,
                               int64_t n_frames) {
  const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (f < n_frames) { stat[f] = 0; tg[f] = 0; fo[f] = 0.0; ifo[f] = 0; }
}

template <typename T>
__global__ void t4_fill_ones_kernel(cx<T>* __restrict__ h, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) h[i] = mk<T>(1, 0);
}

// ofdm_t4_wave.hip
int t4_ifo_wave_launch(const void* rx, const void* tw, int64_t len, int t_guard, int64_t F, int td, const int64_t* tg,
                       const double* fo, int32_t* ifo_out, int32_t* status);
int t4_demod_wave_launch(const void* rx, void* X, const void* tw, int64_t len, int t_guard, int n_symb, int64_t F, int td, int fd,
                         const int64_t* tg, const double* fo, const int32_t* ifo, int n_keep, void* xp, const void* prole, int np);

// One call as its stages see it: shape and route, the caller's buffers, and the regions of the plan arena (t4_arena_layout).
template <typename T>
struct T4Call {
  ofdm_rx_plan* pl;
  T4Shape s;
  T4Route r;
  int64_t F, len, n_out;
  const void* tw;                       // the Nfft-point twiddles
  const cx<T>* rx;
  void* bits; const void* ref; void* errs; void* h_out;
  int64_t* tg; double* fo; int32_t* ifo; int32_t* stat;
  int mer_skip; double* mer;
  const ScopeCall* scope;               // constellation capture (IQ window / density), or null
  int64_t *res, *first;
  double *resv, *est;
  cx<T> *y, *X, *hp, *H, *Xp, *rho, *seg, *spec;
  const cx<T>* pil;                     // the pilot rows fine_sync and the pilot means read: Xp (compact) or X
  const double* rot;                    // est where fine_sync's rotation is applied lazily, else null
};

template <typename T>
static int t4_acf_stage(const T4Call<T>& c) {
  if (c.r.acf == T4_ACF_NONE) return OFDM_OK;
  const int N = c.s.nfft, Tg = c.s.t_guard;
  const int64_t F = c.F, n_out = c.n_out;
  hipStream_t s = ctx().stream;
  if (c.r.acf == T4_ACF_SEARCH) {
    // one workgroup per frame walks the tiles of the autocorrelation until the search of AutoCorrFunction.m:10-20 is
    // decided (t4_acf_search_kernel): no curve in HBM, one launch
    OFDM_HIP(hipFuncSetAttribute((const void*)t4_acf_search_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)acf_search_lds_bytes<T>(ACF_MAXW)));
    hipLaunchKernelGGL(t4_acf_search_kernel<T>, dim3((unsigned)F), dim3(ACF_THREADS), acf_search_lds_bytes<T>(Tg), s, c.rx, c.len,
                       Tg, N, n_out, 0.77, c.tg, c.fo, c.stat);
  } else {
    // OFDM_T4_FULL_ACF: the whole curve per frame, then the search over it (the kernels of ofdm_AutoCorrFunction)
    OFDM_TRY(acf_prepare<T>());
    hipLaunchKernelGGL(acf_kernel<T>, dim3(cdiv_u(n_out, ACF_TILE), (unsigned)F), dim3(ACF_THREADS), acf_lds_bytes<T>(Tg), s, c.rx, c.len, Tg,
                       N, c.rho, n_out, n_out);
    hipLaunchKernelGGL(acf_plateau_kernel<T>, dim3((unsigned)F), dim3(PLAT_THREADS), 0, s, (const cx<T>*)c.rho, n_out, Tg, 0.77,
                       c.res, c.resv, n_out);
    hipLaunchKernelGGL(t4_scalars_kernel, dim3(cdiv_u(F, 256)), dim3(256), 0, s, (const int64_t*)c.res, (const double*)c.resv, n_out,
                       c.tg, c.fo, c.stat, F);
  }
  return check_launch("AutoCorrFunction stage");
}

// staged form: the aligned / corrected copy of the batch first; then the IFO search of remove_IFO.m:5-8
template <typename T>
static int t4_ifo_stage(const T4Call<T>& c) {
  const int N = c.s.nfft, Tg = c.s.t_guard, td = c.s.time_desync, fd = c.s.freq_desync;
  const int64_t F = c.F, len = c.len;
  const bool f64 = std::is_same<T, double>::value;
  hipStream_t s = ctx().stream;
  const unsigned gl = (unsigned)std::min<int64_t>((len + 255) / 256, 64);
  if (c.r.form == T4_FORM_STAGED) {
    hipLaunchKernelGGL(t4_align_kernel<T>, dim3(gl, (unsigned)F), dim3(256), 0, s, c.rx, c.y, len, N + Tg, N, td, fd,
                       (const int64_t*)c.tg, (const double*)c.fo);
    OFDM_TRY(check_launch("t4_align_kernel"));
  }
  if (c.r.ifo == T4_IFO_NONE) return OFDM_OK;
  if (c.r.ifo == T4_IFO_WAVE)                        // segment, spectrum and search in one launch
    return t4_ifo_wave_launch(c.rx, c.tw, len, Tg, F, td, c.tg, c.fo, c.ifo, c.stat);
  if (c.r.ifo == T4_IFO_SEGMENT_DIRECT)              // the segment read from rx through the STO / CFO fix
    hipLaunchKernelGGL(t4_segment_direct_kernel<T>, dim3(cdiv_u(N, 256), (unsigned)F), dim3(256), 0, s, c.rx, c.seg, len, N + Tg, N, td,
                       (const int64_t*)c.tg, (const double*)c.fo);
  else
    hipLaunchKernelGGL(t4_segment_kernel<T>, dim3(cdiv_u(N, 256), (unsigned)F), dim3(256), 0, s, (const cx<T>*)c.y, c.seg, len, N);
  OFDM_TRY(demod_device(c.seg, c.spec, N, F, 0, f64));
  hipLaunchKernelGGL(first_above_kernel<T>, dim3((unsigned)F), dim3(PLAT_THREADS), 0, s, (const cx<T>*)c.spec, (int64_t)N, 0.77, c.first);
  if (c.r.ifo == T4_IFO_SEGMENT_DIRECT)
    hipLaunchKernelGGL(t4_ifo_finalize_kernel, dim3(cdiv_u(F, 256)), dim3(256), 0, s, (const int64_t*)c.first, c.ifo, c.stat, F);
  else
    hipLaunchKernelGGL(t4_ifo_kernel<T>, dim3(gl, (unsigned)F), dim3(256), 0, s, c.y, len, N, (const int64_t*)c.first, c.ifo, c.stat);
  return check_launch("remove_IFO stage");
}

template <typename T>
static int t4_demod_stage(const T4Call<T>& c) {
  const int N = c.s.nfft, Tg = c.s.t_guard, S = c.s.n_symb;
  if (c.r.demod == T4_DEMOD_DEVICE) return demod_device(c.y, c.X, N, (int64_t)S * c.F, Tg, std::is_same<T, double>::value);   // T4:308-310
  auto launch = t4_demod_wave_launch;                // Nfft 2048, fp32, N_carrier <= 1024: one wavefront per symbol run
  if (c.r.demod == T4_DEMOD_NW)
    launch = c.r.nw == 1 ? t4_demod_launch<T, 1> : c.r.nw == 2 ? t4_demod_launch<T, 2> : c.r.nw == 4 ? t4_demod_launch<T, 4> : t4_demod_launch<T, 8>;
  return launch(c.rx, c.X, c.tw, c.len, Tg, S, c.F, c.s.time_desync, c.s.freq_desync, c.tg, c.fo, c.ifo, c.s.n_carrier, c.Xp,
                c.pl->d_prole, c.s.np);
}

// pilot matrix [np x S] = the plan's pilot column on every symbol (T4:28-31) and the spline operator of
// estimate_channel.m:8 for rows 1..N_carrier: built once per plan, kept on the device
template <typename T>
static int t4_plan_tables(ofdm_rx_plan* pl) {
  if (pl->d_t4_tx) return OFDM_OK;
  const int S = pl->n_symb, np = pl->np, nc = pl->n_carrier;
  hipStream_t s = ctx().stream;
  // (the operator first: a plan it refuses -- fewer than two pilots -- is left without tables, and refused again next time)
  std::vector<double> xk(np), xq(nc), W;
  for (int i = 0; i < np; ++i) xk[i] = pl->pilot_loc[i];
  for (int i = 0; i < nc; ++i) xq[i] = i + 1.0;
  OFDM_TRY(build_spline_operator(xk, xq, W));                                       // estimate_channel.m:8, rows 1..N_carrier
  std::vector<cx<T>> col(np), txm((size_t)np * S);
  OFDM_HIP(hipMemcpyAsync(col.data(), pl->d_pilots, sizeof(cx<T>) * np, hipMemcpyDeviceToHost, s));
  OFDM_HIP(hipStreamSynchronize(s));
  for (int sy = 0; sy < S; ++sy) std::copy(col.begin(), col.end(), txm.begin() + (size_t)sy * np);
  OFDM_HIP(hipMalloc(&pl->d_t4_tx, sizeof(cx<T>) * txm.size()));
  OFDM_HIP(hipMemcpy(pl->d_t4_tx, txm.data(), sizeof(cx<T>) * txm.size(), hipMemcpyHostToDevice));
  std::vector<T> Wt(W.begin(), W.end());
  OFDM_HIP(hipMalloc(&pl->d_t4_w, sizeof(T) * Wt.size()));
  OFDM_HIP(hipMemcpy(pl->d_t4_w, Wt.data(), sizeof(T) * Wt.size(), hipMemcpyHostToDevice));
  if (!std::is_same<T, double>::value) {           // fp32: the operator's band (weights below 1e-10 of a row's largest dropped)
    std::vector<float> bw_w;
    std::vector<int32_t> bw_c0;
    mmse_band_spline(W, nc, np, bw_w, bw_c0, pl->t4_bw, pl->t4_span);
    OFDM_HIP(hipMalloc(&pl->d_t4_bw, sizeof(float) * bw_w.size()));
    OFDM_HIP(hipMemcpy(pl->d_t4_bw, bw_w.data(), sizeof(float) * bw_w.size(), hipMemcpyHostToDevice));
    OFDM_HIP(hipMalloc(&pl->d_t4_bc0, sizeof(int32_t) * bw_c0.size()));
    OFDM_HIP(hipMemcpy(pl->d_t4_bc0, bw_c0.data(), sizeof(int32_t) * bw_c0.size(), hipMemcpyHostToDevice));
  }
  return OFDM_OK;
}

// fine_sync (T4:314) and estimate_channel (T4:318)
template <typename T>
static int t4_estimate_stage(const T4Call<T>& c) {
  const ofdm_rx_plan* pl = c.pl;
  const int N = c.s.nfft, S = c.s.n_symb, np = c.s.np, nc = c.s.n_carrier, td = c.s.time_desync, fd = c.s.freq_desync;
  const int64_t F = c.F;
  hipStream_t s = ctx().stream;
  const cx<T>* dtx = (const cx<T>*)pl->d_t4_tx;
  const int32_t* pc0 = (const int32_t*)pl->d_pc0;
  const double deltak = np >= 2 ? (double)pl->pilot_loc[1] - (double)pl->pilot_loc[0] : 1.0;      // fine_sync.m:6
  if (c.r.est == T4_EST_FUSED) {
    // fine_sync's two estimates and the pilot means in ONE launch on the frame's compact pilot rows held in LDS
    OFDM_HIP(hipFuncSetAttribute((const void*)t4_fine_est_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c.r.fine_est_lds));
    hipLaunchKernelGGL(t4_fine_est_kernel<T>, dim3((unsigned)F), dim3(FS_THREADS), c.r.fine_est_lds, s, (const cx<T>*)c.Xp, dtx, pc0, N, np,
                       S, deltak, c.r.sync, td, fd, c.s.mp_desync, c.est, c.hp);
    OFDM_TRY(check_launch("t4_fine_est_kernel"));
  } else if (c.r.est != T4_EST_NONE) {
    PilotView<T> pv{c.pil, dtx, pc0, N, np, (int64_t)np * S, c.r.pilot_fstride, c.r.pilots_compact};
    hipLaunchKernelGGL(fine_tau_kernel<T>, dim3((unsigned)F), dim3(FS_THREADS), 0, s, pv, deltak, 1 /* T4 variant */, c.est);
    hipLaunchKernelGGL(fine_phase_kernel<T>, dim3((unsigned)F), dim3(FS_THREADS), 0, s, pv, td, c.est);
    // staged form: rewrite X; otherwise the rotation is applied where X is read (pilot means, equaliser)
    if (c.r.est == T4_EST_TAU_PHASE_APPLY)
      hipLaunchKernelGGL(fine_apply_kernel<T>, dim3(64, (unsigned)F), dim3(256), 0, s, (const cx<T>*)c.X, c.X, N, (int64_t)S, td, fd,
                         (const double*)c.est);
    OFDM_TRY(check_launch("fine_sync stage"));
  }
  if (c.r.means == T4_MEANS_KERNEL)
    hipLaunchKernelGGL(t4_mean_pilots_kernel<T>, dim3(cdiv_u(np, 128), (unsigned)F), dim3(128), 0, s, c.pil, dtx, pc0, c.hp, N, np, S,
                       c.rot, td, fd, c.r.pilots_compact);
  int dense = c.r.channel == T4_CH_DENSE;
  if (c.r.channel == T4_CH_ONES)
    hipLaunchKernelGGL(t4_fill_ones_kernel<T>, dim3(256), dim3(256), 0, s, c.H, (int64_t)nc * F);
  if (c.r.channel == T4_CH_BAND) {                   // 1: the band does not fit spline_band_kernel's LDS -- the dense product
    dense = spline_band_run((const float*)pl->d_t4_bw, (const int32_t*)pl->d_t4_bc0, pl->t4_bw, pl->t4_span, c.hp, c.H, np, nc, F);
    OFDM_TRY(dense);
  }
  if (dense)
    hipLaunchKernelGGL(t4_apply_operator_kernel<T>, dim3(cdiv_u(nc, 128), cdiv_u(F, T4_FT)), dim3(128), sizeof(cx<T>) * np * T4_FT, s,
                       (const T*)pl->d_t4_w, (const cx<T>*)c.hp, c.H, nc, np, F);
  return check_launch("estimate_channel stage");
}

// equalise, demap and count (T4:334-347, + the sums of MER_func :163); the per-frame DeScrambler of T4:354-364
// (ofdm_rx_plan_set_descrambler) as a pass over the packed decisions
template <typename T>
static int t4_equalise_stage(const T4Call<T>& c) {
  ofdm_rx_plan* pl = c.pl;
  FastPlanView pv;
  make_plan_view(pl, pv);
  pv.ev = nullptr;
  FastParams<T> P;
  OFDM_TRY(fast_params_prepare<T>(pv, c.tw, c.F, P));
  P.h_in = c.H;
  const bool descr_pass = (pl->descr & DESCR_ON) != 0;
  void* craw = nullptr;
  if (descr_pass) OFDM_TRY(descr_raw_workspace(pl, c.F, &craw));
  OFDM_TRY(eq_demap_run<T>(pv, P, (const cx<T>*)c.X, c.r.x_stride, true, c.F, descr_pass ? craw : c.bits, descr_pass ? nullptr : c.ref,
                           descr_pass ? nullptr : c.errs, c.h_out, nullptr, c.rot, c.s.time_desync, c.s.freq_desync, c.mer_skip, c.mer,
                           c.scope));
  if (descr_pass) OFDM_TRY(descr_pass_run(pl, craw, c.bits, c.ref, c.errs, c.F));
  return OFDM_OK;
}

// The call as its stages see it, first half: the route (a refusal before anything is launched or allocated), the frame's extents
// and the caller's buffers.  What the AutoCorrFunction stage on the search route reads; no arena, no table.
template <typename T>
static int t4_call_route(T4Call<T>& c, ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int mp_desync,
                         int64_t* dtg, double* dfo, int32_t* difo, int32_t* dstat) {
  c = T4Call<T>{};
  c.pl = pl; c.F = F;
  c.s = T4Shape{pl->nfft, pl->t_guard, pl->n_symb, pl->n_carrier, pl->np, pl->f64, time_desync, freq_desync, mp_desync, pl->f64 ? 0 : 1};
  const char* why = nullptr;
  OFDM_ARG(t4_route_choose(c.s, c.r, &why) == T4_ROUTE_OK, "%s", why);       // refused before anything is launched or allocated
  c.len = (int64_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  c.n_out = c.len - pl->t_guard - pl->nfft;
  c.rx = (const cx<T>*)drx;
  c.tg = dtg; c.fo = dfo; c.ifo = difo; c.stat = dstat;
  return OFDM_OK;
}

// Second half: the regions of the plan arena, the twiddles and the plan's tables.  The caller fills the outputs behind the front
// end (bits, ref, errs, h_out, mer, scope).
template <typename T>
static int t4_call_prepare(T4Call<T>& c, ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int mp_desync,
                           int64_t* dtg, double* dfo, int32_t* difo, int32_t* dstat) {
  OFDM_TRY(t4_call_route<T>(c, pl, drx, F, time_desync, freq_desync, mp_desync, dtg, dfo, difo, dstat));
  hipStream_t s = ctx().stream;
  // intermediates live in one plan-owned arena (grown on demand): no allocation on the steady-state path
  const T4Arena a = t4_arena_layout(c.s, c.r, F);
  if (pl->ws_t4_bytes < a.total) {
    OFDM_HIP(hipStreamSynchronize(s));
    if (pl->ws_t4) { (void)hipFree(pl->ws_t4); pl->ws_t4 = nullptr; pl->ws_t4_bytes = 0; }
    OFDM_HIP(hipMalloc(&pl->ws_t4, a.total));
    pl->ws_t4_bytes = a.total;
  }
  unsigned char* const arena = (unsigned char*)pl->ws_t4;
  c.res = (int64_t*)(arena + a.res); c.resv = (double*)(arena + a.resv); c.est = (double*)(arena + a.est);
  c.first = (int64_t*)(arena + a.first);
  c.y = (cx<T>*)(arena + a.y); c.X = (cx<T>*)(arena + a.X); c.hp = (cx<T>*)(arena + a.hp); c.H = (cx<T>*)(arena + a.H);
  c.Xp = (cx<T>*)(arena + a.Xp); c.rho = (cx<T>*)(arena + a.rho); c.seg = (cx<T>*)(arena + a.seg); c.spec = (cx<T>*)(arena + a.spec);
  c.pil = c.r.pilots_compact ? c.Xp : c.X;
  c.rot = c.r.lazy_rot ? c.est : nullptr;
  OFDM_TRY(get_twiddles(pl->nfft, pl->f64 != 0, &c.tw));
  OFDM_TRY(t4_plan_tables<T>(pl));
  return OFDM_OK;
}

// The scalars zeroed and AutoCorrFunction (T4:278): TgPosition, FreqOffset and the status (0, 1: the catch branch, -2) of every
// frame.  The first stage of the front end, and what the integer-CFO capture runs in front of its own kernel.
template <typename T>
static int t4_sync_scalars(const T4Call<T>& c) {
  // per-frame scalars start at zero: one launch instead of four memsets (4.7 us each)
  hipLaunchKernelGGL(t4_init_kernel, dim3(cdiv_u(c.F, 256)), dim3(256), 0, ctx().stream, c.stat, c.tg, c.fo, c.ifo, c.F);
  return t4_acf_stage(c);
}

// The front end of the receiver (T4/Main_model_Task_4.m:278-310): the per-frame scalars zeroed, AutoCorrFunction, the two add_STO
// and add_CFO(-FreqOffset), remove_IFO, OFDM_demodulator -- what stands in front of fine_sync.  It leaves X (and, in the direct
// form, the compact pilot rows) in the arena.  mark(i): the stage brackets [0] .. [3] of task4_run.
template <typename T, typename Mark>
static int t4_front_end(const T4Call<T>& c, Mark mark) {
  mark(0);
  OFDM_TRY(t4_sync_scalars(c));
  mark(1);
  OFDM_TRY(t4_ifo_stage(c));
  mark(2);
  OFDM_TRY(t4_demod_stage(c));
  mark(3);
  return OFDM_OK;
}

template <typename T>
static int task4_run(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int mp_desync,
                     void* dbits, const void* dref, void* derr, int64_t* dtg, double* dfo, int32_t* difo, int32_t* dstat,
                     void* dh_out, int mer_skip, double* dmer, const ScopeCall* scope) {
  T4Call<T> c;
  OFDM_TRY(t4_call_prepare<T>(c, pl, drx, F, time_desync, freq_desync, mp_desync, dtg, dfo, difo, dstat));
  c.bits = dbits; c.ref = dref; c.errs = derr; c.h_out = dh_out; c.mer_skip = mer_skip; c.mer = dmer; c.scope = scope;
  hipStream_t s = ctx().stream;
  // stage brackets (ofdm_rx_plan_set_timing): [0] start, [1] AutoCorrFunction stage, [2] remove_IFO stage, [3] demodulator,
  // [4] fine_sync + estimate_channel, [5] equalise / demap / (DeScrambler)
  const bool timed = pl->timing && pl->ev_t4[0];
  pl->t4_timed = timed ? 1 : 0;
  auto mark = [&](int i) { if (timed) (void)hipEventRecord(pl->ev_t4[i], s); };
  OFDM_TRY(t4_front_end(c, mark));
  OFDM_TRY(t4_estimate_stage(c));
  mark(4);
  OFDM_TRY(t4_equalise_stage(c));
  mark(5);
  return OFDM_OK;
}

// The front end alone, for the fine-sync study (ofdm_fine_study.hip): nf frames at drx (device memory, the plan's precision)
// through the stages task4_run runs in front of fine_sync, on the route t4_route_choose gives the receiver for these flags with
// mp_desync 0 (no stage of the front end reads it).  view: where the pilot rows fine_sync reads were left.
template <typename T>
static int t4_front_only(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int64_t* dtg, double* dfo,
                         int32_t* difo, int32_t* dstat, T4PilotRows* view) {
  T4Call<T> c;
  OFDM_TRY(t4_call_prepare<T>(c, pl, drx, F, time_desync, freq_desync, 0, dtg, dfo, difo, dstat));
  OFDM_TRY(t4_front_end(c, [](int) {}));
  view->rows = c.pil;
  view->tx = pl->d_t4_tx;
  view->fstride = c.r.pilot_fstride;
  view->compact = c.r.pilots_compact;
  return OFDM_OK;
}

int task4_front_end(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int64_t* dtg, double* dfo,
                    int32_t* difo, int32_t* dstat, T4PilotRows* view) {
  return pl->f64 ? t4_front_only<double>(pl, drx, F, time_desync, freq_desync, dtg, dfo, difo, dstat, view)
                 : t4_front_only<float>(pl, drx, F, time_desync, freq_desync, dtg, dfo, difo, dstat, view);
}

// The AutoCorrFunction stage alone, for the integer-CFO capture (ofdm_ifo_study.hip): the stage task4_run runs first, on the route
// t4_route_choose gives rx_chain_task4(time_desync, 1, 0), so tg / fo / stat are that call's tg_position_out / freq_offset_out and
// its status before remove_IFO, bit for bit; ifo is zeroed.  The search route needs no arena; with OFDM_T4_FULL_ACF the curve
// lives in the receiver's arena, which is then grown as for a receiver call.
template <typename T>
static int t4_acf_only(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int64_t* dtg, double* dfo, int32_t* difo,
                       int32_t* dstat) {
  T4Call<T> c;
  OFDM_TRY(t4_call_route<T>(c, pl, drx, F, time_desync, 1, 0, dtg, dfo, difo, dstat));
  if (c.r.acf == T4_ACF_FULL) OFDM_TRY(t4_call_prepare<T>(c, pl, drx, F, time_desync, 1, 0, dtg, dfo, difo, dstat));
  return t4_sync_scalars(c);
}

int task4_acf_stage(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int64_t* dtg, double* dfo, int32_t* difo,
                    int32_t* dstat) {
  return pl->f64 ? t4_acf_only<double>(pl, drx, F, time_desync, dtg, dfo, difo, dstat)
                 : t4_acf_only<float>(pl, drx, F, time_desync, dtg, dfo, difo, dstat);
}

// The receiver up to and including estimate_channel, for the channel-estimate capture (ofdm_hest_study.hip): the stages task4_run
// runs in front of the equaliser, on the route t4_route_choose gives rx_chain_task4(time_desync, freq_desync, 1).  view: the
// arena's H -- the equalise stage copies it to h_out unchanged -- and the pilot means the spline operator read.
template <typename T>
static int t4_estimate_only(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int64_t* dtg, double* dfo,
                            int32_t* difo, int32_t* dstat, T4Estimate* view) {
  T4Call<T> c;
  OFDM_TRY(t4_call_prepare<T>(c, pl, drx, F, time_desync, freq_desync, 1, dtg, dfo, difo, dstat));
  OFDM_TRY(t4_front_end(c, [](int) {}));
  OFDM_TRY(t4_estimate_stage(c));
  view->H = c.H;
  view->hp = c.hp;
  return OFDM_OK;
}

int task4_estimate(ofdm_rx_plan* pl, const void* drx, int64_t F, int time_desync, int freq_desync, int64_t* dtg, double* dfo,
                   int32_t* difo, int32_t* dstat, T4Estimate* view) {
  return pl->f64 ? t4_estimate_only<double>(pl, drx, F, time_desync, freq_desync, dtg, dfo, difo, dstat, view)
                 : t4_estimate_only<float>(pl, drx, F, time_desync, freq_desync, dtg, dfo, difo, dstat, view);
}

// the plan's pilot matrix [np x n_symb] on the device (t4_plan_tables), for ofdm_rx_fine
int task4_pilot_matrix(ofdm_rx_plan* pl, const void** tx) {
  OFDM_TRY(pl->f64 ? t4_plan_tables<double>(pl) : t4_plan_tables<float>(pl));
  *tx = pl->d_t4_tx;
  return OFDM_OK;
}

int scope_refused(int id, const ScopeWhy& w) {
  if (id == SCOPE_OK) return OFDM_OK;
  set_error("%s", w.text);
  return OFDM_ERR_ARG;
}

// The body of ofdm_rx_chain_task4_ex / _iq and of the Task-4 sweeps' receiver call.  scope: the capture of this call, or null --
// an IQ window whose iq is where `flags` says (staged like every other output), or a density whose accumulators are device
// memory whatever the flags (ofdm_ber_sweep_task4_scope zeroes and owns them).
int rx_chain_task4_run(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int time_desync, int freq_desync, int mp_desync,
                       uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out, int64_t* tg_position_out,
                       double* freq_offset_out, int32_t* ifo_out, int32_t* status_out, void* h_out, int64_t mer_skip,
                       double* mer_sums_out, const ScopeCall* scope, int flags) {
  OFDM_TRY(ensure_init());
  OFDM_ARG(pl && rx && n_frames >= 0, "rx_chain_task4: bad arguments");
  OFDM_ARG(pl->nd >= 1, "rx_chain_task4: the plan has no data carriers");
  OFDM_ARG(mer_skip >= 0 && mer_skip < (int64_t)pl->nd * pl->n_symb,
           "rx_chain_task4_ex: mer_skip must be 0 .. nd * N_symb - 1 (%lld)", (long long)mer_skip);
  if (scope && scope->iq) {
    ScopeWhy why;
    OFDM_TRY(scope_refused(scope_iq_check(scope->iq_first, scope->iq_count, (int64_t)pl->nd * pl->n_symb, why), why));
  }
  OFDM_PLAN_DEVICE(pl);
  OFDM_ARG((is_f64(flags) ? 1 : 0) == pl->f64, "rx_chain_task4: precision flag differs from the plan's");
  OFDM_ARG(pl->pilots_in_band, "rx_chain_task4: pilots outside 1..N_carrier are not supported");
  OFDM_ARG(!errors_out || ref_bits, "rx_chain_task4: errors_out needs ref_bits");
  OFDM_ARG(n_frames <= 65535, "rx_chain_task4: at most 65535 frames per call");
  if (n_frames == 0) return OFDM_OK;
  const size_t cs = csize(flags);
  const size_t frame_samples = (size_t)(pl->nfft + pl->t_guard) * pl->n_symb;
  const size_t fb = (size_t)pl->frame_words * 4;
  Stage st(flags);
  const void *drx, *dref; void *dbits, *derr, *dtg, *dfo, *difo, *dstat, *dh;
  OFDM_TRY(st.in(rx, cs * frame_samples * n_frames, &drx));
  OFDM_TRY(st.in(ref_bits, fb * n_frames, &dref));
  OFDM_TRY(st.out(bits_out, fb * n_frames, &dbits));
  OFDM_TRY(st.out(errors_out, sizeof(uint32_t) * n_frames, &derr));
  OFDM_TRY(st.out(h_out, cs * (size_t)pl->n_carrier * n_frames, &dh));
  // the per-frame scalars are always produced (scratch when the caller does not want them)
  if (tg_position_out) OFDM_TRY(st.out(tg_position_out, sizeof(int64_t) * n_frames, &dtg)); else OFDM_TRY(st.scratch(sizeof(int64_t) * n_frames, &dtg));
  if (freq_offset_out) OFDM_TRY(st.out(freq_offset_out, sizeof(double) * n_frames, &dfo)); else OFDM_TRY(st.scratch(sizeof(double) * n_frames, &dfo));
  if (ifo_out) OFDM_TRY(st.out(ifo_out, sizeof(int32_t) * n_frames, &difo)); else OFDM_TRY(st.scratch(sizeof(int32_t) * n_frames, &difo));
  if (status_out) OFDM_TRY(st.out(status_out, sizeof(int32_t) * n_frames, &dstat)); else OFDM_TRY(st.scratch(sizeof(int32_t) * n_frames, &dstat));
  void* dmer;
  OFDM_TRY(st.out(mer_sums_out, sizeof(double) * 2 * n_frames, &dmer));
  ScopeCall sc;
  if (scope) {
    sc = *scope;
    if (sc.iq) OFDM_TRY(st.out(scope->iq, cs * (size_t)sc.iq_count * n_frames, &sc.iq));
  }
  const ScopeCall* dsc = scope ? &sc : nullptr;
  if (pl->f64)
    OFDM_TRY(task4_run<double>(pl, drx, n_frames, time_desync, freq_desync, mp_desync, dbits, dref, derr, (int64_t*)dtg, (double*)dfo,
                               (int32_t*)difo, (int32_t*)dstat, dh, (int)mer_skip, (double*)dmer, dsc));
  else
    OFDM_TRY(task4_run<float>(pl, drx, n_frames, time_desync, freq_desync, mp_desync, dbits, dref, derr, (int64_t*)dtg, (double*)dfo,
                              (int32_t*)difo, (int32_t*)dstat, dh, (int)mer_skip, (double*)dmer, dsc));
  return st.finish();
}

}  // namespace ofdm

using namespace ofdm;

extern "C" {

int ofdm_rx_chain_task4_ex(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int time_desync, int freq_desync, int mp_desync,
                           uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out, int64_t* tg_position_out,
                           double* freq_offset_out, int32_t* ifo_out, int32_t* status_out, void* h_out, int64_t mer_skip,
                           double* mer_sums_out, int flags) {
  return rx_chain_task4_run(pl, rx, n_frames, time_desync, freq_desync, mp_desync, bits_out, ref_bits, errors_out, tg_position_out,
                            freq_offset_out, ifo_out, status_out, h_out, mer_skip, mer_sums_out, nullptr, flags);
}

int ofdm_rx_chain_task4_iq(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int time_desync, int freq_desync, int mp_desync,
                           uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out, int64_t* tg_position_out,
                           double* freq_offset_out, int32_t* ifo_out, int32_t* status_out, void* h_out, int64_t mer_skip,
                           double* mer_sums_out, int64_t iq_first, int64_t iq_count, void* iq_out, int flags) {
  ScopeCall sc;
  sc.iq_first = iq_first; sc.iq_count = iq_count; sc.iq = iq_out;
  return rx_chain_task4_run(pl, rx, n_frames, time_desync, freq_desync, mp_desync, bits_out, ref_bits, errors_out, tg_position_out,
                            freq_offset_out, ifo_out, status_out, h_out, mer_skip, mer_sums_out, iq_out ? &sc : nullptr, flags);
}

int ofdm_rx_chain_task4(ofdm_rx_plan* pl, const void* rx, int64_t n_frames, int time_desync, int freq_desync, int mp_desync,
                        uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out, int64_t* tg_position_out,
                        double* freq_offset_out, int32_t* ifo_out, int32_t* status_out, void* h_out, int flags) {
  return ofdm_rx_chain_task4_ex(pl, rx, n_frames, time_desync, freq_desync, mp_desync, bits_out, ref_bits, errors_out,
                                tg_position_out, freq_offset_out, ifo_out, status_out, h_out, 0, nullptr, flags);
}

}  // extern "C"
