// The error anatomy: where the wrong bits of a batch of packed decisions sit -- per data carrier, per OFDM symbol, per bit of the
// constellation label, as distances between neighbouring errors of a frame, per frame and on the time-frequency grid.  What every
// BER of the reference ends in is one number (T3/Main_model_Task_3.m:237-266, T4/Main_model_Task_4.m:354-366); behind its
// self-synchronising DeScrambler (T5/DeScrambler.m:8-13) one channel error is three payload errors, at i, i + 13 and i + 14.
//
//   bit_error_profile_kernel<MAP>  workgroup b walks the frames b, b + grid, ..  A frame is read in tiles of 256 consecutive words,
//                                  one word per lane and coalesced: decisions XOR reference, byte-swapped to stream order (as
//                                  descr_pass_kernel reads them), the padding of the last word masked.  Every set bit bumps the
//                                  LDS counters carrier[nd], symbol[N_symb], label[bps]; its position (s, d, r) comes from one
//                                  division per word that has an error and a running update per bit (err_position, err_advance:
//                                  error_plan.hpp).  The gap to the error in front of it needs the last error position in front of
//                                  each word: every lane keeps the last set bit of its word, a max-scan over the wavefront and the
//                                  four wavefronts orders them, a carry runs from tile to tile.  Per frame the error count (a
//                                  butterfly, the four wave partials) goes to frame_errors.  The LDS tables are flushed once per
//                                  workgroup with 64-bit global atomics; the host keeps a workgroup's frames below the count that
//                                  could wrap a 32-bit counter (err_pass).  MAP: the time-frequency map by global atomics, one per
//                                  erroneous QAM symbol of a word.  One corner leaves "no global traffic per bit but the map":
//                                  where symbol[N_symb] does not fit in LDS beside the other tables (N_symb beyond about 7000)
//                                  the symbol counts go to the global table, one 64-bit atomic per OFDM symbol a word touches
//                                  (a run of the word's errors in one symbol is one atomic, as for the map).
// Integers added in no particular order: every output is bitwise independent of the chunking and of the grid.
// ofdm_error_study generates each chunk with the fused generator (txf_sweep_points), runs the Task-5 or the Task-4 receiver on it as
// the matching sweep does (rx_chain_task5_run, rx_chain_task4_run: untouched) with bits_out in a chunk buffer, and profiles that
// buffer.  side = channel: the plan's DeScrambler is masked for the call (DescrMask restores it on every return path), so the
// receiver writes its raw decisions, which are compared against the scrambled bits.  Host side: the checks, the chunk and the
// launch shape are error_plan.hpp's.
#include <algorithm>
#include <cmath>

#include "error_plan.hpp"
#include "txf_study.hpp"

namespace ofdm {

struct ErrGeom {
  int nd, n_symb, bps, frame_words, gap_bins, symbols_in_lds;
  int64_t frame_bits;
  uint32_t recip;            // err_recip(bps)
};

// the accumulators of one point (all but frame_errors and map are always there)
struct ErrTables {
  unsigned long long *errors, *frames_in_error, *carrier, *symbol, *label, *gap_hist, *gap_above, *map;
  uint32_t* frame_errors;
};

template <bool MAP>
__global__ __launch_bounds__(ERR_THREADS) void bit_error_profile_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ ref,
                                                                        int64_t nf, ErrGeom g, ErrTables o) {
  extern __shared__ __align__(16) uint32_t lds[];
  // the scan's scratch in front (64-bit aligned), the counters behind it in the order of err_lds_bytes
  long long* const wave_last = reinterpret_cast<long long*>(lds);            // [2][ERR_WAVES]
  uint32_t* const wave_err = lds + 4 * ERR_WAVES;                            // [ERR_WAVES]
  uint32_t* const carrier = lds + ERR_SCRATCH_WORDS;
  uint32_t* const symbol = carrier + g.nd;
  uint32_t* const label = symbol + (g.symbols_in_lds ? g.n_symb : 0);
  uint32_t* const gap = label + g.bps;                                       // [gap_bins + 1], the last: above
  const int n_counters = g.nd + (g.symbols_in_lds ? g.n_symb : 0) + g.bps + g.gap_bins + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < n_counters; i += ERR_THREADS) carrier[i] = 0;
  __syncthreads();
  unsigned long long total = 0, in_error = 0;                                // thread 0's
  int par = 0;
  for (int64_t f = blockIdx.x; f < nf; f += gridDim.x) {
    const uint32_t* const fb = bits + f * g.frame_words;
    const uint32_t* const fr = ref + f * g.frame_words;
    long long carry = -1;                                                    // the frame's last error in front of the tile
    uint32_t ferr = 0;
    for (int w0 = 0; w0 < g.frame_words; w0 += ERR_THREADS) {
      const int w = w0 + tid;
      uint32_t x = 0;
      if (w < g.frame_words) {
        x = __builtin_bswap32(fb[w] ^ fr[w]);                                // stream order: MSB first
        // frame_words = ceil(frame_bits / 32) (the plan's invariant, checked before the launch): valid >= 1 for every word
        const int64_t valid = g.frame_bits - (int64_t)w * 32;
        if (valid < 32) x &= ~(0xffffffffu >> (int)valid);
      }
      ferr += __popc(x);
      // the last error of the frame in front of this word: an inclusive max-scan of the lanes' last set bits
      long long v = x ? (long long)w * 32 + (32 - __ffs((int)x)) : -1;
      for (int off = 1; off < 64; off <<= 1) {
        const long long t = __shfl_up(v, off, 64);
        if (lane >= off) v = v > t ? v : t;
      }
      long long prev = __shfl_up(v, 1, 64);
      if (lane == 0) prev = -1;
      if (lane == 63) wave_last[par * ERR_WAVES + wave] = v;
      __syncthreads();
      long long next = carry;
      for (int k = 0; k < ERR_WAVES; ++k) {
        const long long t = wave_last[par * ERR_WAVES + k];
        if (k < wave) carry = carry > t ? carry : t;
        next = next > t ? next : t;
      }
      prev = prev > carry ? prev : carry;
      carry = next;
      par ^= 1;                                                              // the next tile writes the other half: one barrier per tile
      if (x) {
        const int64_t i0 = (int64_t)w * 32;
        ErrPos p = err_position(i0, g.nd, g.bps);                            // the divisions: once per word that has an error
        int at = 0;
        int64_t ms = -1;                                                     // MAP: the QAM symbol being counted
        int md = 0;
        unsigned long long mc = 0;
        int64_t gs = -1;                                                     // symbol table in global memory: the run being counted
        unsigned long long gc = 0;
        while (x) {
          const int b = __clz((int)x);
          x &= ~(0x80000000u >> b);
          err_advance(p, b - at, g.nd, g.bps, g.recip);
          at = b;
          atomicAdd(&carrier[p.d], 1u);
          if (g.symbols_in_lds) {
            atomicAdd(&symbol[p.s], 1u);
          } else {                                                           // one global atomic per OFDM symbol a word touches
            if (p.s != gs) {
              if (gc) atomicAdd(&o.symbol[gs], gc);
              gs = p.s; gc = 0;
            }
            ++gc;
          }
          atomicAdd(&label[p.r], 1u);
          const long long i = i0 + b;
          if (prev >= 0) {
            const long long d = i - prev;
            atomicAdd(&gap[d <= g.gap_bins ? (int)d - 1 : g.gap_bins], 1u);
          }
          prev = i;
          if constexpr (MAP) {
            if (p.s != ms || p.d != md) {
              if (mc) atomicAdd(&o.map[ms * g.nd + md], mc);
              ms = p.s; md = p.d; mc = 0;
            }
            ++mc;
          }
        }
        if constexpr (MAP) { if (mc) atomicAdd(&o.map[ms * g.nd + md], mc); }
        if (gc) atomicAdd(&o.symbol[gs], gc);
      }
    }
    for (int off = 32; off > 0; off >>= 1) ferr += __shfl_xor(ferr, off, 64);
    if (lane == 0) wave_err[wave] = ferr;
    __syncthreads();                                                         // (the next write of wave_err is behind a tile's barrier)
    if (tid == 0) {
      uint32_t e = 0;
      for (int k = 0; k < ERR_WAVES; ++k) e += wave_err[k];
      if (o.frame_errors) o.frame_errors[f] = e;
      total += e;
      in_error += e ? 1 : 0;
    }
  }
  __syncthreads();
  for (int i = tid; i < n_counters; i += ERR_THREADS) {
    const uint32_t c = carrier[i];
    if (!c) continue;
    int k = i;
    unsigned long long* dst;
    if (k < g.nd) dst = o.carrier + k;
    else if ((k -= g.nd) < (g.symbols_in_lds ? g.n_symb : 0)) dst = o.symbol + k;
    else if ((k -= (g.symbols_in_lds ? g.n_symb : 0)) < g.bps) dst = o.label + k;
    else dst = (k -= g.bps) < g.gap_bins ? o.gap_hist + k : o.gap_above;
    atomicAdd(dst, (unsigned long long)c);
  }
  if (tid == 0) {
    if (total) atomicAdd(o.errors, total);
    if (in_error) atomicAdd(o.frames_in_error, in_error);
  }
}

// the tables of nf frames added to o; launches of at most grid * flush_frames frames (err_pass)
static int err_profile_frames(const TxfShape& s, int gap_bins, const uint32_t* bits, const uint32_t* ref, int64_t nf, const ErrTables& o) {
  const ErrGeom g{s.nd, s.n_symb, s.bps, s.frame_words, gap_bins, 0, err_frame_bits(s), err_recip(s.bps)};
  if ((int64_t)s.frame_words != (g.frame_bits + 31) / 32) {             // what the kernel's padding mask and its word loop assume
    set_error("bit_error_profile_kernel: the plan's frame has %d words for %lld bits", s.frame_words, (long long)g.frame_bits);
    return OFDM_ERR_STATE;
  }
  for (int64_t f0 = 0; f0 < nf;) {
    const ErrPass p = err_pass(s, gap_bins, nf - f0);
    if (p.threads != ERR_THREADS || p.lds > ERR_LDS_LIMIT || p.launch_frames < 1 ||
        (p.launch_frames + p.grid - 1) / p.grid > p.flush_frames) {
      set_error("bit_error_profile_kernel: launch shape differs from the kernel's");
      return OFDM_ERR_STATE;
    }
    ErrGeom gl = g;
    gl.symbols_in_lds = p.symbols_in_lds;
    ErrTables ol = o;
    if (ol.frame_errors) ol.frame_errors += f0;
    const uint32_t* const b = bits + f0 * s.frame_words;
    const uint32_t* const r = ref + f0 * s.frame_words;
    if (o.map)
      hipLaunchKernelGGL(bit_error_profile_kernel<true>, dim3(p.grid), dim3(p.threads), p.lds, ctx().stream, b, r, p.launch_frames, gl, ol);
    else
      hipLaunchKernelGGL(bit_error_profile_kernel<false>, dim3(p.grid), dim3(p.threads), p.lds, ctx().stream, b, r, p.launch_frames, gl, ol);
    OFDM_TRY(check_launch("bit_error_profile_kernel"));
    f0 += p.launch_frames;
  }
  return OFDM_OK;
}

// the outputs of both entries for n points: the tables a caller did not ask for are still summed (scratch): the same kernel,
// whatever the outputs; frame_errors and map only when asked for.  All zeroed on the launch stream.
struct ErrOutputs {
  unsigned long long *errors, *fie, *carrier, *symbol, *label, *gap_hist, *gap_above;
  void *frame_errors, *map;
  size_t nd, ns, bps, gb;
  // the tables of point p; frame: the sweep index of the first frame counted (p * frames_per_point + its index in the point)
  ErrTables point(size_t p, size_t frame) const {
    return ErrTables{errors + p, fie + p, carrier + p * nd, symbol + p * ns, label + p * bps, gap_hist + p * gb, gap_above + p,
                     map ? (unsigned long long*)map + p * ns * nd : nullptr,
                     frame_errors ? (uint32_t*)frame_errors + frame : nullptr};
  }
};

static int err_outputs(Stage& st, const TxfShape& s, int gap_bins, size_t n_points, size_t frames_per_point, uint64_t* errors_out,
                       uint64_t* frames_in_error_out, uint64_t* carrier_out, uint64_t* symbol_out, uint64_t* label_out,
                       uint64_t* gap_hist_out, uint64_t* gap_above_out, uint32_t* frame_errors_out, uint64_t* map_out, ErrOutputs& o) {
  o.nd = (size_t)s.nd; o.ns = (size_t)s.n_symb; o.bps = (size_t)s.bps; o.gb = (size_t)gap_bins;
  const size_t one = sizeof(uint64_t);
  OFDM_TRY(txf_table(st, errors_out, n_points, o.errors));
  OFDM_TRY(txf_table(st, frames_in_error_out, n_points, o.fie));
  OFDM_TRY(txf_table(st, carrier_out, o.nd * n_points, o.carrier));
  OFDM_TRY(txf_table(st, symbol_out, o.ns * n_points, o.symbol));
  OFDM_TRY(txf_table(st, label_out, o.bps * n_points, o.label));
  OFDM_TRY(txf_table(st, gap_hist_out, o.gb * n_points, o.gap_hist));
  OFDM_TRY(txf_table(st, gap_above_out, n_points, o.gap_above));
  OFDM_TRY(st.out(frame_errors_out, sizeof(uint32_t) * frames_per_point * n_points, &o.frame_errors));
  OFDM_TRY(st.out(map_out, one * o.ns * o.nd * n_points, &o.map));
  if (o.map) OFDM_HIP(hipMemsetAsync(o.map, 0, one * o.ns * o.nd * n_points, ctx().stream));
  return OFDM_OK;
}

// the plan's DeScrambler masked while the study's receiver calls run, put back on every return path
struct DescrMask {
  ofdm_rx_plan* pl;
  uint32_t saved;
  DescrMask(ofdm_rx_plan* pl_, bool mask) : pl(pl_), saved(pl_->descr) { if (mask) pl->descr = 0; }
  ~DescrMask() { pl->descr = saved; }
  DescrMask(const DescrMask&) = delete;
  DescrMask& operator=(const DescrMask&) = delete;
};

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_bit_error_profile(ofdm_rx_plan* pl, const uint8_t* bits, const uint8_t* ref_bits, int64_t n_frames, int gap_bins,
                                      uint64_t* errors_out, uint64_t* frames_in_error_out, uint64_t* carrier_out, uint64_t* symbol_out,
                                      uint64_t* label_out, uint64_t* gap_hist_out, uint64_t* gap_above_out, uint32_t* frame_errors_out,
                                      uint64_t* map_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  ErrTablesWanted want;
  want.gap_bins = gap_bins;
  want.out = errors_out || frames_in_error_out || carrier_out || symbol_out || label_out || gap_hist_out || gap_above_out ||
             frame_errors_out || map_out;
  TxfWhy why;
  OFDM_TRY(txf_refused(err_profile_prelude(pl ? &s : nullptr, bits != nullptr, ref_bits != nullptr, n_frames, want, why), why));
  Stage st(flags);
  const size_t fb = sizeof(uint32_t) * (size_t)s.frame_words * (size_t)n_frames;
  const void *dbits = nullptr, *dref = nullptr;
  if (n_frames > 0) {
    OFDM_TRY(st.in(bits, fb, &dbits));
    OFDM_TRY(st.in(ref_bits, fb, &dref));
  }
  ErrOutputs o{};
  OFDM_TRY(err_outputs(st, s, gap_bins, 1, (size_t)n_frames, errors_out, frames_in_error_out, carrier_out, symbol_out, label_out,
                       gap_hist_out, gap_above_out, frame_errors_out, map_out, o));
  if (n_frames > 0) OFDM_TRY(err_profile_frames(s, gap_bins, (const uint32_t*)dbits, (const uint32_t*)dref, n_frames, o.point(0, 0)));
  return st.finish();
}

extern "C" int ofdm_error_study(ofdm_rx_plan* pl, int receiver, const void* h, int h_len, const int32_t* tap_delay,
                                const double* tap_power, int n_taps, int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                                int time_desync, int freq_desync, int mp_desync, const double* snr_db, const uint64_t* seeds,
                                int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15, int side,
                                int gap_bins, int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* frames_in_error_out,
                                uint64_t* carrier_out, uint64_t* symbol_out, uint64_t* label_out, uint64_t* gap_hist_out,
                                uint64_t* gap_above_out, uint32_t* frame_errors_out, uint64_t* map_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs g{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, frames_per_point, frame0, max_frames_per_chunk, flags};
  const bool fading = g.fading();
  // the refusals of the matching sweep come in its own words: the call is named as that sweep names itself
  TxfCall c = g.call(receiver == 4 ? (fading ? "ber_sweep_task4_fading" : "ber_sweep_task4")
                                   : (fading ? "ber_sweep_task5_fading" : "ber_sweep_task5"), pl ? &s : nullptr);
  c.out = true;                                                  // (the study's own outputs are checked last)
  c.mp_desync = mp_desync;
  ErrStudyArgs a;
  a.receiver = receiver; a.side = side; a.both_channels = g.both_channels();
  a.time_desync = time_desync; a.freq_desync = freq_desync; a.mp_desync = mp_desync;
  ErrTablesWanted want;
  want.gap_bins = gap_bins;
  want.out = errors_out || frames_in_error_out || carrier_out || symbol_out || label_out || gap_hist_out || gap_above_out ||
             frame_errors_out || map_out;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(err_study_prelude(c, a, want, ch, fade.gains, why), why));
  if (n_points == 0) return OFDM_OK;
  Stage st(flags);
  ErrOutputs o{};
  OFDM_TRY(err_outputs(st, s, gap_bins, (size_t)n_points, (size_t)frames_per_point, errors_out, frames_in_error_out, carrier_out,
                       symbol_out, label_out, gap_hist_out, gap_above_out, frame_errors_out, map_out, o));
  if (frames_per_point == 0) return st.finish();
  const bool scr = scr_reg15 != nullptr;
  const bool channel_side = side == 1 && scr;                    // without a Register the two sides are the same bits
  const int taps = (int)ch.delay.size();
  const TxfUse u = err_use(receiver, scr, fading ? taps : 0);
  const int64_t CH = err_chunk(s, u, receiver, frames_per_point, max_frames_per_chunk);
  const size_t chn = (size_t)CH, wb = sizeof(uint32_t) * (size_t)s.frame_words;
  void *dec, *scref = nullptr, *dtg = nullptr, *dfo = nullptr, *difo = nullptr, *dstat = nullptr;
  OFDM_TRY(st.scratch(wb * chn, &dec));
  if (channel_side) OFDM_TRY(st.scratch(wb * chn, &scref));
  if (receiver == 4) {
    OFDM_TRY(st.scratch(sizeof(int64_t) * chn, &dtg));
    OFDM_TRY(st.scratch(sizeof(double) * chn, &dfo));
    OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &difo));
    OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &dstat));
  }
  const TxfImp imp = g.imp();                                    // receiver 4: the draws of the chunk's frames, as the sweep's
  TxfPoints pt = g.points(true);
  pt.scref = (uint32_t*)scref;
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  // behind every check that reads the plan's DeScrambler (the workspace the loop sets up in front of its first chunk reads none)
  const DescrMask mask(pl, channel_side);
  OFDM_TRY(txf_sweep_points(pl, ch, pt, scr_reg15, CH, receiver == 4 ? &imp : nullptr, fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    if (receiver == 4) {
      OFDM_TRY(rx_chain_task4_run(pl, b.rx, nf, time_desync, freq_desync, mp_desync, (uint8_t*)dec, nullptr, nullptr, (int64_t*)dtg,
                                  (double*)dfo, (int32_t*)difo, (int32_t*)dstat, nullptr, 0, nullptr, nullptr, rxflags));
    } else {
      const double inv_snr = 1.0 / std::pow(10.0, snr_db[p] * 0.1);         // (as ofdm_ber_sweep_task5 passes it: h = ifft(H_LS) mode)
      OFDM_TRY(rx_chain_task5_run(pl, b.rx, nf, (uint8_t*)dec, nullptr, nullptr, nullptr, nullptr, nullptr, rxflags, inv_snr));
    }
    return err_profile_frames(s, gap_bins, (const uint32_t*)dec, channel_side ? (const uint32_t*)scref : b.ref, nf,
                              o.point((size_t)p, (size_t)at));
  }));
  return st.finish();
}
