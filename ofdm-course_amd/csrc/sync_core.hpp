// Device code of the receiver synchronisation that the per-function entries (ofdm_sync.hip) and the batched Task-4 receiver
// (ofdm_chain_t4.hip) share: the autocorrelation tile and curve, the plateau and threshold searches, fine_sync's reductions
// and kernels.
#pragma once

#include "rx_plan.hpp"

namespace ofdm {

static unsigned ew_grid(int64_t total, int per_block = 256) {
  int64_t b = (total + per_block - 1) / per_block;
  int64_t cap = (int64_t)ctx().num_cu * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// ---------------------------------------------------------------------------------------------
// AutoCorrFunction.m:3-7.  rho(n) = sum_W x[m] conj(x[m+N]) / sqrt(sum_W |x[m]|^2 * sum_W |x[m+N]|^2)
// for every n.  The reference is O(L*W); here each workgroup owns a tile of ACF_TILE outputs, forms
// the three running sums as tile-local exclusive prefix sums in LDS (double accumulation: every thread
// scans its own run of <= 8 consecutive products serially, ONE wave-shuffle scan of the 256 run totals
// ties them together) and takes S[n+W]-S[n]: O(L) work, each sample read twice (once as x[m], once as
// x[m+N]) and rho written once.
// ---------------------------------------------------------------------------------------------
constexpr int ACF_TILE = 1024;
constexpr int ACF_THREADS = 256;
constexpr int ACF_MAXW = 1024;                       // WidthWindow limit (T_guard <= 1024 <-> Nfft <= 8192)
constexpr int ACF_ELEMS = ACF_TILE + ACF_MAXW;       // prefix entries 0..ACF_ELEMS
constexpr int ACF_DIRECT_W = 8;                      // windows below the shortest guard interval (Nfft 64) are summed directly

// accumulation type A: double in parity mode; float in fp32 mode (tile-local prefixes of <= 2048 terms: the window sums
// keep ~1e-6 relative accuracy, the fp32 tolerance of rho is 1e-4) -- 16-byte table entries, 20 KB per workgroup instead of
// 64 KB (seven resident workgroups per CU instead of two) and a float square root / reciprocal per output
template <typename A> struct acf4 { A pr, pi, e1, e2; };

template <typename A> __device__ __forceinline__ acf4<A> acf_add(acf4<A> a, acf4<A> b) { return acf4<A>{a.pr + b.pr, a.pi + b.pi, a.e1 + b.e1, a.e2 + b.e2}; }
template <typename A> __device__ __forceinline__ acf4<A> acf_shfl_up(acf4<A> v, int d) {
  return acf4<A>{__shfl_up(v.pr, d, 64), __shfl_up(v.pi, d, 64), __shfl_up(v.e1, d, 64), __shfl_up(v.e2, d, 64)};
}
template <typename T> inline size_t acf_lds_bytes(int W) { return sizeof(acf4<T>) * (size_t)(ACF_TILE + W + 1); }

// One tile of ACF_TILE outputs starting at n0 of one stream x: emit(i, rho) for i < n_here.  All ACF_THREADS threads call it;
// S = the dynamic LDS table, wtot = ACF_THREADS / 64 entries of static LDS.  Ends with the table still valid (the caller
// synchronises before the next tile overwrites it).
template <typename T, typename Emit>
__device__ __forceinline__ void acf_tile(const cx<T>* __restrict__ x, int64_t n0, int n_here, int W, int nfft,
                                         acf4<T>* __restrict__ S, acf4<T>* __restrict__ wtot, Emit emit) {
  using A = T;
  using acc = acf4<A>;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int m_cnt = n_here + W - 1;                  // elements needed: m = n0 .. n0+n_here+W-2
  // (1) every thread forms the products of its own run of E consecutive elements and their inclusive prefix in
  //     registers (a wavefront still reads one contiguous span of x; the lines are reused across the run) ...
  constexpr int EMAX = ACF_ELEMS / ACF_THREADS;                   // 8
  const int E = (m_cnt + ACF_THREADS - 1) / ACF_THREADS;          // <= EMAX
  const int lo_i = tid * E;
  acc pre[EMAX];
  acc run{0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < EMAX; ++j) {
    const int i = lo_i + j;
    if (j < E && i < m_cnt) {
      const int64_t m = n0 + i;                      // m + nfft < len is guaranteed by n_out
      const cx<T> a = x[m], b = x[m + nfft];
      const A ar = a.x, ai = a.y, br = b.x, bi = b.y;
      run = acf_add(run, acc{ar * br + ai * bi,      // a * conj(b)
                             ai * br - ar * bi, ar * ar + ai * ai, br * br + bi * bi});
    }
    pre[j] = run;
  }
  // (2) ... one exclusive scan of the 256 run totals (wave shuffle scan + carry of the earlier wavefronts) ...
  acc v = run;
  for (int d = 1; d < 64; d <<= 1) {
    acc u = acf_shfl_up(v, d);
    if (lane >= d) v = acf_add(v, u);
  }
  if (lane == 63) wtot[wid] = v;
  if (tid == 0) S[0] = acc{0, 0, 0, 0};
  __syncthreads();
  acc off{0, 0, 0, 0};
  for (int w = 0; w < wid; ++w) off = acf_add(off, wtot[w]);
  off = acf_add(off, acc{v.pr - run.pr, v.pi - run.pi, v.e1 - run.e1, v.e2 - run.e2});
  // (3) ... and the prefix table is written once: S[i+1] = sum_{m <= i}
#pragma unroll
  for (int j = 0; j < EMAX; ++j) {
    const int i = lo_i + j;
    if (j < E && i < m_cnt) S[i + 1] = acf_add(pre[j], off);
  }
  __syncthreads();
  for (int i = tid; i < n_here; i += ACF_THREADS) {
    const acc hi = S[i + W], lo = S[i];
    A pr = hi.pr - lo.pr, pi = hi.pi - lo.pi, e1 = hi.e1 - lo.e1, e2 = hi.e2 - lo.e2;
    if (W < ACF_DIRECT_W) {
      // A window of a few samples is a small part of the tile's prefix, and a weak sample loses its digits in the difference
      // (WidthWindow 1, double: 5e-11 in |rho| against the 1e-11 this library holds rho to): its sums are taken from x.
      pr = pi = e1 = e2 = A(0);
      const cx<T>* const xa = x + n0 + i;              // m + nfft < len as in (1)
      for (int k = 0; k < W; ++k) {
        const cx<T> a = xa[k], b = xa[k + nfft];
        const A ar = a.x, ai = a.y, br = b.x, bi = b.y;
        pr += ar * br + ai * bi; pi += ai * br - ar * bi; e1 += ar * ar + ai * ai; e2 += br * br + bi * bi;
      }
    }
    // A window of zeros (the tail add_STO leaves, a late frame's head) is 0 / 0 = NaN in the reference, "not above" in :10-12.
    // The table is not bitwise constant over a run of zeros that crosses a thread boundary (tree scan of the run totals), so
    // the difference can be a rounding residue instead of 0: an energy within the table's rounding of zero is looked at.
    const A tiny = A(256) * std::numeric_limits<A>::epsilon();
    if (e1 <= tiny * hi.e1 || e2 <= tiny * hi.e2) {
      bool za = true, zb = true;
      const cx<T>* const xa = x + n0 + i;            // m + nfft < len as in (1)
      for (int k = 0; k < W; ++k) {
        const cx<T> a = xa[k], b = xa[k + nfft];
        za = za && a.x == T(0) && a.y == T(0);
        zb = zb && b.x == T(0) && b.y == T(0);
      }
      if (za || zb) { pr = pi = A(0); if (za) e1 = A(0); if (zb) e2 = A(0); }
    }
    const A den = sqrt(e1 * e2);                     // AutoCorrFunction.m:6
    if constexpr (sizeof(A) == 4) {
      const A inv = A(1) / den;
      emit(i, mk<T>(pr * inv, pi * inv));
    } else {
      emit(i, mk<T>((T)(pr / den), (T)(pi / den)));
    }
  }
}

template <typename T>
__global__ __launch_bounds__(ACF_THREADS) void acf_kernel(const cx<T>* __restrict__ x, int64_t len, int W, int nfft,
                                                          cx<T>* __restrict__ rho, int64_t n_out, int64_t rho_stride = 0) {
  // batched callers: grid.y = frame (one stream per frame); rho rows rho_stride apart (0: n_out)
  using acc = acf4<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char acf_smem[];
  acc* const S = (acc*)acf_smem;                     // [ACF_TILE + W + 1] exclusive prefix: S[i] = sum_{m<i}
  __shared__ acc wtot[ACF_THREADS / 64];
  const int64_t fr = blockIdx.y;
  x += fr * len;
  rho += fr * (rho_stride ? rho_stride : n_out);
  const int64_t n0 = (int64_t)blockIdx.x * ACF_TILE;
  const int n_here = (int)((n_out - n0 < ACF_TILE) ? (n_out - n0) : ACF_TILE);
  cx<T>* const dst = rho + n0;
  acf_tile<T>(x, n0, n_here, W, nfft, S, wtot, [dst](int i, cx<T> r) { dst[i] = r; });
}

// dynamic LDS beyond 64 KB (double table at WidthWindow = 1024) has to be allowed for the kernel (per device: set on every call)
template <typename T>
static int acf_prepare() {
  OFDM_HIP(hipFuncSetAttribute((const void*)acf_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)acf_lds_bytes<T>(ACF_MAXW)));
  return OFDM_OK;
}

// ---------------------------------------------------------------------------------------------
// AutoCorrFunction.m:10-24 -- threshold 0.77, indices > WidthWindow, first run of consecutive
// indices; needs a second run to exist (result(2)) or the catch branch gives 65.
// One workgroup scans in chunks with early exit.  out[0]=TgPosition (1-based), out[1]=ok,
// outv[0..1] = rho(TgPosition).
// ---------------------------------------------------------------------------------------------
constexpr int PLAT_THREADS = 1024;

template <typename T, typename Pred>
__device__ int64_t first_index_where(const cx<T>* __restrict__ rho, int64_t from, int64_t n, Pred pred, int64_t* sh) {
  // returns the smallest i in [from, n) with pred(i), or -1; all threads must call
  for (int64_t base = from; base < n; base += PLAT_THREADS) {
    const int64_t i = base + threadIdx.x;
    const bool hit = (i < n) && pred(rho[i]);
    if (threadIdx.x == 0) *sh = INT64_MAX;
    __syncthreads();
    if (hit) atomicMin((unsigned long long*)sh, (unsigned long long)i);
    __syncthreads();
    const int64_t r = *sh;
    __syncthreads();
    if (r != INT64_MAX) return r;
  }
  return -1;
}

template <typename T>
__global__ __launch_bounds__(PLAT_THREADS) void acf_plateau_kernel(const cx<T>* __restrict__ rho, int64_t n, int W,
                                                                   double thr, int64_t* __restrict__ out,
                                                                   double* __restrict__ outv, int64_t rho_stride = 0) {
  rho += (int64_t)blockIdx.x * (rho_stride ? rho_stride : n);   // grid.x = frame
  out += 2 * blockIdx.x;
  outv += 2 * blockIdx.x;
  __shared__ int64_t sh;
  auto above = [thr](cx<T> v) { return sqrt((double)v.x * v.x + (double)v.y * v.y) > thr; };
  auto below = [thr](cx<T> v) { return !(sqrt((double)v.x * v.x + (double)v.y * v.y) > thr); };
  int64_t pos = 65;                                   // AutoCorrFunction.m:23
  int ok = 0;
  // 1-based index idx = i+1 must satisfy idx > W  <=>  i >= W
  const int64_t f = first_index_where<T>(rho, W, n, above, &sh);
  if (f >= 0) {
    const int64_t g = first_index_where<T>(rho, f + 1, n, below, &sh);      // run 1 = [f, g-1]
    if (g >= 0) {
      const int64_t h = first_index_where<T>(rho, g + 1, n, above, &sh);    // a second run exists
      if (h >= 0) {
        pos = ((f + 1) + (g - 1 + 1)) / 2;                                   // :20 floor of the mean of 1-based ends
        ok = 1;
      }
    }
  }
  if (threadIdx.x == 0) {
    out[0] = pos;
    out[1] = ok;
    if (pos >= 1 && pos <= n) { outv[0] = rho[pos - 1].x; outv[1] = rho[pos - 1].y; }
    else { outv[0] = NAN; outv[1] = NAN; }
  }
}

// first spectral bin with |X| > thr (remove_IFO.m:6-8); out[0] = 0-based bin or -1
template <typename T>
__global__ __launch_bounds__(PLAT_THREADS) void first_above_kernel(const cx<T>* __restrict__ spec, int64_t n, double thr,
                                                                   int64_t* __restrict__ out) {
  spec += (int64_t)blockIdx.x * n;                   // grid.x = frame
  out += blockIdx.x;
  __shared__ int64_t sh;
  auto above = [thr](cx<T> v) { return sqrt((double)v.x * v.x + (double)v.y * v.y) > thr; };
  const int64_t f = first_index_where<T>(spec, 0, n, above, &sh);
  if (threadIdx.x == 0) out[0] = f;
}

// ---------------------------------------------------------------------------------------------
// fine_sync.m:10-20 -- residual timing estimate.  Pilots of all symbols flattened column-major
// (M = Np*S); taus(i) = angle(q(i+1) conj(q(i)))/(2 pi dk), taus(M)=0; keep where
// |taus(i)-taus(i-1)| < 1e-3; tau = mean of the kept values after dropping the first Np KEPT ones.
// Single workgroup, chunked, with a running rank (ballot prefix count).  angle(0) := 0.
// ---------------------------------------------------------------------------------------------
constexpr int FS_THREADS = 256;

__device__ __forceinline__ double angle0(double re, double im) { return (re == 0.0 && im == 0.0) ? 0.0 : atan2(im, re); }
// angle of a pilot product: parity mode in double; throughput mode (fp32 data) with the float atan2 -- the double one is
// ~150 double-rate instructions and made the two fine-sync reductions compute-bound once their gathers were gone
template <typename T>
__device__ __forceinline__ double angle0_t(double re, double im) {
  if constexpr (sizeof(T) == 4) return (re == 0.0 && im == 0.0) ? 0.0 : (double)atan2f((float)im, (float)re);
  else return angle0(re, im);
}

template <typename T>
struct PilotView {
  const cx<T>* rx;          // [nfft x n_symb]
  const cx<T>* tx;          // [np x n_symb]
  const int32_t* pc0;       // 0-based pilot rows
  int nfft, np;
  int64_t M;                // np * n_symb, < 2^31 (checked on the host)
  int64_t rx_fstride;       // elements between the frames of a batch (0 for a single frame)
  int compact;              // rx is already X(pilotCarriers, :) = [np x n_symb] (the batched receiver: written by its demodulator)
  __device__ void q(unsigned i, double& qr, double& qi) const {    // q = tx * conj(rx)
    const unsigned s = i / (unsigned)np, p = i - s * (unsigned)np;
    const cx<T> r = compact ? rx[i] : rx[(size_t)s * nfft + pc0[p]];
    const cx<T> t = tx[i];
    qr = (double)t.x * r.x + (double)t.y * r.y;
    qi = (double)t.y * r.x - (double)t.x * r.y;
  }
};

// taus(i) = angle(q(i+1) conj(q(i))) / (2 pi dk)
template <typename T>
__device__ __forceinline__ double tau_of(double ar, double ai, double br, double bi, double inv2pidk) {
  return angle0_t<T>(br * ar + bi * ai, bi * ar - br * ai) * inv2pidk;
}

// Every thread owns FS_U CONSECUTIVE entries of `taus` per trip: their FS_U + 2 pilot products are requested together
// (the kernel is bound by the latency of these gathers, not by arithmetic: one workgroup per frame), each product and
// each angle is formed once, and a frame of 6700 pilots takes 7 trips instead of 27.
constexpr int FS_U = 4;

// scratch of the two reductions (static LDS of the calling kernel)
struct FsScratch {
  int wcnt[FS_THREADS / 64];
  double wsum[FS_THREADS / 64];
  int64_t wn[FS_THREADS / 64];
  double result;
};

// What the two reductions leave behind beside their estimate.  FsNoCapture, the default, is nothing: the receiver's and
// ofdm_fine_sync's instantiations are the code they were.  FsCapture (fine_capture_kernel, ofdm_fine_study.hip): every entry of
// `taus` (fine_sync.m:14, before the mask) and its keep flag (:18 / T4 :33) go to the frame's rows in the trip that forms them, and
// the two denominators -- the kept entries behind the first Np kept ones (:20), the angles above 1e-3 (:37) -- are written once.
struct FsNoCapture {
  static constexpr bool on = false;
};
struct FsCapture {
  static constexpr bool on = true;
  double* taus;              // [L], or null
  uint8_t* keep;             // [L], or null
  int32_t* n_used;           // [1]
  int32_t* n_phase;          // [1]
};

// the residual timing estimate tau of one frame, returned to every thread of the FS_THREADS-thread workgroup
template <typename T, typename Cap = FsNoCapture>
__device__ double fine_tau_body(const PilotView<T>& pv, double deltak, int variant, FsScratch& sc, Cap cap = Cap{}) {
  int (&wcnt)[FS_THREADS / 64] = sc.wcnt;
  double (&wsum)[FS_THREADS / 64] = sc.wsum;
  int64_t (&wn)[FS_THREADS / 64] = sc.wn;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const double inv = 1.0 / (2.0 * M_PI * deltak);
  const unsigned M = (unsigned)pv.M;
  int64_t rank_base = 0;       // kept elements before this trip
  double sum = 0.0;
  int64_t cnt = 0;
  // length of `taus`: T5/fine_sync.m:8 allocates numel(pilotValues) entries (the loop leaves the last one 0);
  // T4/fine_sync.m:8 allocates Np and lets the loop of :25-30 grow it to numel-1 entries -- no trailing 0
  const unsigned L = (variant == 1 && pv.M - 1 >= pv.np) ? M - 1 : M;
  for (unsigned base = 0; base < L; base += FS_THREADS * FS_U) {
    const unsigned i0 = base + FS_U * tid;                       // entries i0 .. i0 + FS_U - 1
    // products q(i0 - 1) .. q(i0 + FS_U): taus(i) needs q(i), q(i + 1); the first difference needs taus(i0 - 1)
    double qr[FS_U + 2], qi[FS_U + 2];
#pragma unroll
    for (int u = 0; u < FS_U + 2; ++u) {
      const long long i = (long long)i0 + u - 1;
      qr[u] = qi[u] = 0.0;
      if (i >= 0 && i < (long long)M && i0 < L) pv.q((unsigned)i, qr[u], qi[u]);
    }
    double tp = 0.0;                                             // taus(i0 - 1)
    if (i0 >= 1 && i0 - 1 < M - 1) tp = tau_of<T>(qr[0], qi[0], qr[1], qi[1], inv);
    bool keep[FS_U];
    double tv[FS_U];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < FS_U; ++u) {
      const unsigned i = i0 + u;
      keep[u] = false;
      tv[u] = 0.0;
      if (i < L) {
        tv[u] = i < M - 1 ? tau_of<T>(qr[u + 1], qi[u + 1], qr[u + 2], qi[u + 2], inv) : 0.0;      // taus(M) = 0 (T5 form)
        if (i >= 1) {
          const double d = tv[u] - tp;
          keep[u] = fabs(d) < 1e-3;                              // fine_sync.m:18
          if (variant == 1) keep[u] = keep[u] && (d != 0.0);     // T4/fine_sync.m:33
        }
      }
      tp = tv[u];
      mine += keep[u] ? 1 : 0;
      if constexpr (Cap::on) {
        if (i < L) {
          if (cap.taus) cap.taus[i] = tv[u];
          if (cap.keep) cap.keep[i] = keep[u] ? 1 : 0;
        }
      }
    }
    // rank among the kept entries, in entry order (thread-major, then u)
    int before = 0, wtot = 0;
#pragma unroll
    for (int u = 0; u < FS_U; ++u) {
      const unsigned long long bal = __ballot(keep[u]);
      before += __popcll(bal & ((1ull << lane) - 1ull));
      wtot += __popcll(bal);
    }
    if (lane == 0) wcnt[wid] = wtot;
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < FS_THREADS / 64; ++w) { if (w < wid) woff += wcnt[w]; tot += wcnt[w]; }
    int64_t rank = rank_base + woff + before;                    // 0-based rank of this thread's first kept entry
#pragma unroll
    for (int u = 0; u < FS_U; ++u)
      if (keep[u]) {
        if (rank >= pv.np) { sum += tv[u]; cnt += 1; }           // :20 taus_result(Np+1:end)
        rank += 1;
      }
    rank_base += tot;
    __syncthreads();
  }
  for (int off = 32; off > 0; off >>= 1) { sum += __shfl_down(sum, off, 64); cnt += __shfl_down(cnt, off, 64); }
  if (lane == 0) { wsum[wid] = sum; wn[wid] = cnt; }
  __syncthreads();
  if (tid == 0) {
    double s = 0; int64_t n = 0;
    for (int w = 0; w < FS_THREADS / 64; ++w) { s += wsum[w]; n += wn[w]; }
    sc.result = n > 0 ? s / (double)n : NAN;                     // mean([]) = NaN
    if constexpr (Cap::on) *cap.n_used = (int32_t)n;
  }
  __syncthreads();
  const double r = sc.result;
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(FS_THREADS) void fine_tau_kernel(PilotView<T> pv, double deltak, int variant,
                                                              double* __restrict__ out /* [0]=tau */) {
  pv.rx += (int64_t)blockIdx.x * pv.rx_fstride;      // grid.x = frame
  __shared__ FsScratch sc;
  const double tau = fine_tau_body<T>(pv, deltak, variant, sc);
  if (threadIdx.x == 0) out[2 * blockIdx.x] = tau;
}

// fine_sync.m:32-37 -- common phase after the (optional) timing derotation; out[1] = phase_shift
// rotation exp(-2 pi j tau k) of pilot row k as (cos, sin): the arithmetic of fine_phase_body's per-entry form
template <typename T>
__device__ __forceinline__ void fine_rot(double tau, int k, double& cs, double& sn) {
  const double t = tau * (double)k;
  if constexpr (sizeof(T) == 4) {                                  // throughput mode: phase reduced in double, sine / cosine in float
    float fs, fc;
    sincospif(2.0f * (float)(t - floor(t)), &fs, &fc);
    sn = fs; cs = fc;
  } else {
    sincospi(2.0 * (t - floor(t)), &sn, &cs);
  }
}

// rot_tab (optional, [np] (cos, sin) of fine_rot per pilot row): the rotation depends on the pilot row only, a caller that
// holds a whole frame computes it once per row instead of once per (row, symbol) -- same values
template <typename T, typename Cap = FsNoCapture>
__device__ double fine_phase_body(const PilotView<T>& pv, int time_desync, double tau, FsScratch& sc,
                                  const double2* rot_tab = nullptr, Cap cap = Cap{}) {
  double (&wsum)[FS_THREADS / 64] = sc.wsum;
  int64_t (&wn)[FS_THREADS / 64] = sc.wn;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned M = (unsigned)pv.M;
  // i mod np by a multiply (exact while i * np < 2^32: frames of up to 65535 pilot samples), else the division
  const unsigned npu = (unsigned)pv.np, magic = (M < 65536u && npu < 65536u) ? 0xFFFFFFFFu / npu + 1u : 0u;
  auto mod_np = [&](unsigned i) { return magic ? i - __umulhi(i, magic) * npu : i % npu; };
  double sum = 0.0;
  int64_t cnt = 0;
  for (unsigned base = 0; base < M; base += FS_THREADS * FS_U) {
    double qr[FS_U], qi[FS_U];
#pragma unroll
    for (int u = 0; u < FS_U; ++u) {                              // FS_U gathers in flight per thread
      const unsigned i = base + u * FS_THREADS + tid;
      qr[u] = qi[u] = 0.0;
      if (i < M) pv.q(i, qr[u], qi[u]);
    }
#pragma unroll
    for (int u = 0; u < FS_U; ++u) {
      const unsigned i = base + u * FS_THREADS + tid;
      if (i < M) {
        if (time_desync) {
          // rx' = rx * exp(+2 pi j tau k)  =>  q' = q * exp(-2 pi j tau k)   (fine_sync.m:25-27, nn_exp')
          double sn, cs;
          if (rot_tab) { const double2 r = rot_tab[mod_np(i)]; cs = r.x; sn = r.y; }
          else fine_rot<T>(tau, pv.pc0[mod_np(i)], cs, sn);
          const double r2 = qr[u] * cs + qi[u] * sn, i2 = qi[u] * cs - qr[u] * sn;
          qr[u] = r2; qi[u] = i2;
        }
        const double a = angle0_t<T>(qr[u], qi[u]);              // :35
        if (fabs(a) > 1e-3) { sum += a; cnt += 1; }              // :37
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) { sum += __shfl_down(sum, off, 64); cnt += __shfl_down(cnt, off, 64); }
  if (lane == 0) { wsum[wid] = sum; wn[wid] = cnt; }
  __syncthreads();
  if (tid == 0) {
    double s = 0; int64_t n = 0;
    for (int w = 0; w < FS_THREADS / 64; ++w) { s += wsum[w]; n += wn[w]; }
    sc.result = n > 0 ? s / (double)n : NAN;
    if constexpr (Cap::on) *cap.n_phase = (int32_t)n;
  }
  __syncthreads();
  const double r = sc.result;
  __syncthreads();
  return r;
}

template <typename T>
__global__ __launch_bounds__(FS_THREADS) void fine_phase_kernel(PilotView<T> pv, int time_desync,
                                                                double* __restrict__ out) {
  pv.rx += (int64_t)blockIdx.x * pv.rx_fstride;      // grid.x = frame
  __shared__ FsScratch sc;
  const double ph = fine_phase_body<T>(pv, time_desync, out[2 * blockIdx.x], sc);
  if (threadIdx.x == 0) out[2 * blockIdx.x + 1] = ph;
}

// fine_sync.m:23-29,:39-43 -- apply both corrections in one pass
template <typename T>
__global__ void fine_apply_kernel(const cx<T>* __restrict__ x, cx<T>* __restrict__ y, int nfft, int64_t n_symb,
                                  int time_desync, int freq_desync, const double* __restrict__ est) {
  x += (int64_t)blockIdx.y * nfft * n_symb;          // grid.y = frame
  y += (int64_t)blockIdx.y * nfft * n_symb;
  est += 2 * blockIdx.y;
  const double tau = est[0], ph = est[1];
  double psn = 0.0, pcs = 1.0;
  if (freq_desync) sincos(ph, &psn, &pcs);
  const int64_t total = (int64_t)nfft * n_symb;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % nfft);
    double cs = 1.0, sn = 0.0;
    if (time_desync) {
      const double t = tau * (double)k;
      sincospi(2.0 * (t - floor(t)), &sn, &cs);
    }
    // total rotation = exp(j(2 pi tau k + ph))
    const double rc = cs * pcs - sn * psn, rs = sn * pcs + cs * psn;
    const cx<T> v = x[i];
    y[i] = mk<T>((T)((double)v.x * rc - (double)v.y * rs), (T)((double)v.x * rs + (double)v.y * rc));
  }
}

}  // namespace ofdm
