// The payload transport: the caller's bits through the fused generator and a receiver, and back as one stream -- what every driver
// of the reference does before its curves (file_reader.m -> the chain -> DeScrambler -> BER_func -> display_pic.m;
// T3/Main_model_Task_3.m:26-32, :160-185, the same lines in T1, T2, T4, T5).
//
// The stream is packed as the library packs bits: stream bit i is bit 7 - i % 8 of byte i / 8.  It is cut into frames of
// frame_bits = nd N_symb bps bits, in general no multiple of 8: a frame's first bit sits anywhere in a byte.  The receivers return
// a frame's decisions padded to whole 32-bit words; joined back, two frames (and two chunks) meet inside one word of the stream.
// A word of the stream read as big-endian holds 32 consecutive stream bits, MSB first, so 32 bits from any bit position on are one
// funnel shift of two neighbouring words (pay_stream32); where a frame sits in the stream is payload_position (payload_plan.hpp).
//
//   payload_frames_kernel   the way in, per chunk.  Item = one packed word of a frame: the funnel shift, the bits beyond the frame's
//                           share of the payload masked to 0 (the padding display_pic.m:5-6 assumes), stored in the receivers'
//                           layout (ref).  Item = one 16-byte group of the chunk's byte-per-bit region (b0: what
//                           ofdm_Scrambler_frames and tx_symbols_fused_kernel read): its 16 bits from one funnel shift (more where
//                           a frame ends inside the group), spread to bytes, one 16-byte store.  Coalesced in both, no loop over
//                           bits in global memory.  The group behind the chunk's last bit is written whole: b0 must be padded to
//                           16 bytes (the workspace pads every region to 256).
//   payload_join_kernel     the way out, per chunk.  Item = one packed word of a frame's decisions: masked to the frame's share,
//                           shifted to its bit offset in the stream of its repeat, OR-ed into the one or two words it covers
//                           (integer atomics on zeroed memory: two frames, or two chunks, that meet in a word each add their own
//                           bits, in any order).  The rows of the staging stream are whole words; the caller's rows of
//                           ceil(n_bits / 8) bytes are copied from them at the end of the call.
//   payload_tally_kernel    per chunk.  A workgroup per frame: popcount(decisions ^ payload) over the frame's share in a fixed
//                           order, to frame_errors and (64-bit atomic) to the errors of the frame's repeat.  With `ones`, further
//                           workgroups own one stream bit per thread: the sum of that decoded bit over the chunk's repeats of its
//                           frame, added to the column (neighbouring threads read the same word and write neighbouring columns).
// Integers only: every output is bitwise independent of the chunking.
//
// ofdm_payload_transport generates each chunk with the fused generator (txf_sweep_points with the payload as its bit source), runs
// the Task-5 or the Task-4 receiver on it as the matching sweep does (rx_chain_task5_run, rx_chain_task4_run: untouched), joins and
// tallies.  Host side: the checks, the number of frames, the chunk and the launch shapes are payload_plan.hpp's.
#include <algorithm>
#include <cmath>

#include "payload_plan.hpp"
#include "txf_study.hpp"

namespace ofdm {

// 32 stream bits from stream bit s on, MSB first.  words: the staged stream, a zero word behind its last
__device__ __forceinline__ uint32_t pay_stream32(const uint32_t* __restrict__ words, int64_t s) {
  const int64_t k = s >> 5;
  const uint32_t hi = __builtin_bswap32(words[k]), lo = __builtin_bswap32(words[k + 1]);
  return __funnelshift_l(lo, hi, (uint32_t)(s & 31));
}

__device__ __forceinline__ uint32_t pay_mask(int valid) { return valid >= 32 ? 0xffffffffu : ~(0xffffffffu >> valid); }

// the 32 bits of a frame at `pos` from frame bit i0 on, MSB first; what is not payload is 0
__device__ __forceinline__ uint32_t pay_frame32(const uint32_t* __restrict__ words, const PayloadPos& pos, int64_t i0) {
  const int valid = payload_valid(pos, i0);
  return valid ? pay_stream32(words, pos.bit0 + i0) & pay_mask(valid) : 0u;
}

// four bits (MSB first) as four bytes in memory order
__device__ __forceinline__ uint32_t pay_spread4(uint32_t n) {
  return ((n >> 3) & 1u) | (((n >> 2) & 1u) << 8) | (((n >> 1) & 1u) << 16) | ((n & 1u) << 24);
}

__global__ __launch_bounds__(PAY_THREADS) void payload_frames_kernel(const uint32_t* __restrict__ words, PayloadCut cut, int64_t frame,
                                                                     int64_t nf, int frame_words, uint8_t* __restrict__ b0,
                                                                     uint32_t* __restrict__ ref) {
  const int64_t n_ref = ref ? nf * frame_words : 0;
  const int64_t n_grp = (nf * cut.frame_bits + 15) / 16;
  const int64_t stride = (int64_t)gridDim.x * PAY_THREADS;
  for (int64_t item = (int64_t)blockIdx.x * PAY_THREADS + threadIdx.x; item < n_ref + n_grp; item += stride) {
    if (item < n_ref) {
      const int64_t j = item / frame_words;
      const int64_t w = item - j * frame_words;
      ref[item] = __builtin_bswap32(pay_frame32(words, payload_position(cut, frame + j), w * 32));
      continue;
    }
    const int64_t q0 = (item - n_ref) * 16;                       // the group's first bit, counted over the chunk
    int64_t j = q0 / cut.frame_bits;
    int64_t i = q0 - j * cut.frame_bits;
    uint32_t bits = 0;                                            // 16 bits, the first in bit 15
    int have = 0;
    while (have < 16 && j < nf) {
      const int64_t left = cut.frame_bits - i;
      const int take = left < 16 - have ? (int)left : 16 - have;  // 1 .. 16
      const uint32_t v = pay_frame32(words, payload_position(cut, frame + j), i);
      bits |= (v >> (32 - take)) << (16 - have - take);
      have += take;
      i += take;
      if (i == cut.frame_bits) { i = 0; ++j; }
    }
    uint4 o;
    o.x = pay_spread4(bits >> 12);
    o.y = pay_spread4(bits >> 8);
    o.z = pay_spread4(bits >> 4);
    o.w = pay_spread4(bits);
    *reinterpret_cast<uint4*>(b0 + q0) = o;
  }
}

// dec: the chunk's decisions [nf][frame_words]; stream: the point's staging rows [repeats][row_words], zeroed before the first chunk
__global__ __launch_bounds__(PAY_THREADS) void payload_join_kernel(const uint32_t* __restrict__ dec, PayloadCut cut, int64_t frame,
                                                                   int64_t nf, int frame_words, int64_t row_words,
                                                                   uint32_t* __restrict__ stream) {
  const int64_t stride = (int64_t)gridDim.x * PAY_THREADS;
  for (int64_t item = (int64_t)blockIdx.x * PAY_THREADS + threadIdx.x; item < nf * frame_words; item += stride) {
    const int64_t j = item / frame_words;
    const int64_t i0 = (item - j * frame_words) * 32;
    const PayloadPos pos = payload_position(cut, frame + j);
    const int valid = payload_valid(pos, i0);
    if (!valid) continue;
    const uint32_t v = __builtin_bswap32(dec[item]) & pay_mask(valid);
    if (!v) continue;
    const int64_t d = pos.bit0 + i0;
    const int sh = (int)(d & 31);
    uint32_t* const row = stream + pos.repeat * row_words + (d >> 5);
    atomicOr(row, __builtin_bswap32(v >> sh));
    // (bits behind the word's end are payload bits: the row has a word for them)
    if (sh && (v << (32 - sh))) atomicOr(row + 1, __builtin_bswap32(v << (32 - sh)));
  }
}

// errors [repeats], frame_errors [repeats F] (optional), ones [n_bits] (optional): the point's; the first frame_blocks workgroups
// take the frames, the others (with ones) the columns
__global__ __launch_bounds__(PAY_THREADS) void payload_tally_kernel(const uint32_t* __restrict__ dec, const uint32_t* __restrict__ ref,
                                                                    PayloadCut cut, int64_t frame, int64_t nf, int frame_words,
                                                                    unsigned frame_blocks, unsigned long long* __restrict__ errors,
                                                                    uint32_t* __restrict__ frame_errors, uint32_t* __restrict__ ones) {
  __shared__ uint32_t wave_err[PAY_THREADS / 64];
  const int tid = threadIdx.x;
  if (blockIdx.x < frame_blocks) {
    for (int64_t j = blockIdx.x; j < nf; j += frame_blocks) {
      const PayloadPos pos = payload_position(cut, frame + j);
      uint32_t e = 0;
      for (int w = tid; w < frame_words; w += PAY_THREADS) {
        const int valid = payload_valid(pos, (int64_t)w * 32);
        if (valid) e += __popc(__builtin_bswap32(dec[j * frame_words + w] ^ ref[j * frame_words + w]) & pay_mask(valid));
      }
      for (int off = 32; off > 0; off >>= 1) e += __shfl_xor(e, off, 64);
      if ((tid & 63) == 0) wave_err[tid >> 6] = e;
      __syncthreads();
      if (tid == 0) {
        uint32_t t = 0;
        for (int k = 0; k < PAY_THREADS / 64; ++k) t += wave_err[k];
        if (frame_errors) frame_errors[frame + j] = t;
        if (t) atomicAdd(errors + pos.repeat, (unsigned long long)t);
      }
      __syncthreads();
    }
    return;
  }
  if (!ones) return;
  const int64_t stride = (int64_t)(gridDim.x - frame_blocks) * PAY_THREADS;
  for (int64_t col = (int64_t)(blockIdx.x - frame_blocks) * PAY_THREADS + tid; col < cut.n_bits; col += stride) {
    const int64_t pf = col / cut.frame_bits;
    const int64_t i = col - pf * cut.frame_bits;
    int64_t g = frame / cut.period * cut.period + pf;             // the chunk's first repeat of payload frame pf
    if (g < frame) g += cut.period;
    uint32_t sum = 0;
    for (; g < frame + nf; g += cut.period)
      sum += (__builtin_bswap32(dec[(g - frame) * frame_words + (i >> 5)]) >> (31 - (int)(i & 31))) & 1u;
    // a plain read-modify-write: one thread owns a column in a launch, and the launches of a point run in order on one stream
    if (sum) ones[col] += sum;
  }
}

static PayloadCut pay_cut(const ofdm_rx_plan* pl, const TxfPayload& src) {
  return PayloadCut{src.n_bits, (int64_t)pl->nd * pl->n_symb * pl->bps, src.first_frame, src.period};
}

int payload_stage(Stage& st, const uint8_t* payload, int64_t n_bits, const uint32_t** words) {
  const size_t given = (size_t)payload_bytes(n_bits), staged = payload_staged_bytes(n_bits);
  const void* src = nullptr;
  void* d = nullptr;
  OFDM_TRY(st.in(payload, given, &src));
  OFDM_TRY(st.scratch(staged, &d));
  // the stream's last word and the word behind it zeroed, then the bytes there are (staged >= 8, given <= staged - 4)
  OFDM_HIP(hipMemsetAsync((unsigned char*)d + staged - 8, 0, 8, ctx().stream));
  OFDM_HIP(hipMemcpyAsync(d, src, given, hipMemcpyDeviceToDevice, ctx().stream));
  *words = (const uint32_t*)d;
  return OFDM_OK;
}

int payload_frames_device(const ofdm_rx_plan* pl, const TxfPayload& src, int64_t nf, uint8_t* b0, uint32_t* ref) {
  if (nf == 0) return OFDM_OK;
  if (!(src.words && b0)) {
    set_error("payload_frames_kernel: no stream, or no byte-per-bit region in the workspace");
    return OFDM_ERR_STATE;
  }
  const int64_t items = payload_cut_items(txf_shape(pl), nf, ref != nullptr);
  hipLaunchKernelGGL(payload_frames_kernel, dim3(payload_grid(items)), dim3(PAY_THREADS), 0, ctx().stream, src.words, pay_cut(pl, src),
                     src.frame, nf, pl->frame_words, b0, ref);
  return check_launch("payload_frames_kernel");
}

}  // namespace ofdm

using namespace ofdm;

extern "C" int ofdm_payload_transport(ofdm_rx_plan* pl, int receiver, const uint8_t* payload, int64_t n_bits, int64_t repeats,
                                      const void* h, int h_len, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                      int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                                      int freq_desync, int mp_desync, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                      int64_t frame0, const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint8_t* decoded_out,
                                      uint64_t* errors_out, uint32_t* frame_errors_out, uint32_t* ones_out, int flags) {
  OFDM_TRY(ensure_init());
  const TxfShape s = pl ? txf_shape(pl) : TxfShape{};
  const TxfStudyArgs g{h, h_len, tap_delay, tap_power, n_taps, sto_mode, sto_value, cfo_mode, cfo_value, scr_reg15, snr_db, seeds,
                       n_points, 0, frame0, max_frames_per_chunk, flags};
  const bool fading = g.fading();
  TxfCall c = g.call("transport", pl ? &s : nullptr);
  c.out = true;                                                  // (the transport's own outputs are checked last)
  c.mp_desync = mp_desync;
  PayTransportArgs a;
  a.receiver = receiver; a.payload = payload != nullptr; a.both_channels = g.both_channels();
  a.out = decoded_out || errors_out || frame_errors_out || ones_out;
  a.n_bits = n_bits; a.repeats = repeats;
  a.time_desync = time_desync; a.freq_desync = freq_desync; a.mp_desync = mp_desync;
  TxfChannel ch;
  TxfFade fade;
  TxfWhy why;
  OFDM_TRY(txf_refused(payload_transport_prelude(c, a, ch, fade.gains, why), why));
  if (n_points == 0) return OFDM_OK;
  const int64_t frame_bits = (int64_t)s.nd * s.n_symb * s.bps;
  const int64_t F = payload_frames(n_bits, frame_bits), FR = c.n_frames;
  const size_t P = (size_t)n_points, R = (size_t)repeats;
  const size_t row_words = (size_t)payload_words(n_bits), row_bytes = (size_t)payload_bytes(n_bits);
  Stage st(flags);
  hipStream_t stream = ctx().stream;
  TxfPayload src;
  OFDM_TRY(payload_stage(st, payload, n_bits, &src.words));
  src.n_bits = n_bits;
  src.period = F;
  const PayloadCut cut{n_bits, frame_bits, 0, F};
  unsigned long long* derr = nullptr;
  void *dfe = nullptr, *dones = nullptr, *ddec = nullptr, *rows = nullptr;
  OFDM_TRY(txf_table(st, errors_out, P * R, derr));
  OFDM_TRY(st.out(frame_errors_out, sizeof(uint32_t) * P * (size_t)FR, &dfe));            // every frame writes its own
  OFDM_TRY(st.out(ones_out, sizeof(uint32_t) * P * (size_t)n_bits, &dones));
  if (dones) OFDM_HIP(hipMemsetAsync(dones, 0, sizeof(uint32_t) * P * (size_t)n_bits, stream));
  OFDM_TRY(st.out(decoded_out, P * R * row_bytes, &ddec));
  if (ddec) {
    OFDM_TRY(st.scratch(sizeof(uint32_t) * P * R * row_words, &rows));
    OFDM_HIP(hipMemsetAsync(rows, 0, sizeof(uint32_t) * P * R * row_words, stream));
  }
  const bool scr = scr_reg15 != nullptr;
  const TxfUse u = payload_use(receiver, scr, fading ? (int)ch.delay.size() : 0);
  const int64_t CH = payload_chunk(s, u, receiver, FR, max_frames_per_chunk);
  const size_t chn = (size_t)CH, wb = sizeof(uint32_t) * (size_t)s.frame_words;
  void *dec, *dtg = nullptr, *dfo = nullptr, *difo = nullptr, *dstat = nullptr;
  OFDM_TRY(st.scratch(wb * chn, &dec));
  if (receiver == 4) {
    OFDM_TRY(st.scratch(sizeof(int64_t) * chn, &dtg));
    OFDM_TRY(st.scratch(sizeof(double) * chn, &dfo));
    OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &difo));
    OFDM_TRY(st.scratch(sizeof(int32_t) * chn, &dstat));
  }
  const TxfImp imp = g.imp();                                    // receiver 4: the draws of the chunk's frames, as the sweep's
  TxfPoints pt{snr_db, seeds, n_points, FR, frame0, true};
  pt.payload = &src;
  const int rxflags = OFDM_DEVICE | (pl->f64 ? OFDM_F64 : 0);
  OFDM_TRY(txf_sweep_points(pl, ch, pt, scr_reg15, CH, receiver == 4 ? &imp : nullptr, fading ? &fade : nullptr, u,
                            [&](const TxfBuffers& b, int64_t nf, int64_t p, int64_t at) -> int {
    if (receiver == 4) {
      OFDM_TRY(rx_chain_task4_run(pl, b.rx, nf, time_desync, freq_desync, mp_desync, (uint8_t*)dec, nullptr, nullptr, (int64_t*)dtg,
                                  (double*)dfo, (int32_t*)difo, (int32_t*)dstat, nullptr, 0, nullptr, nullptr, rxflags));
    } else {
      const double inv_snr = 1.0 / std::pow(10.0, snr_db[p] * 0.1);         // (as ofdm_ber_sweep_task5 passes it: h = ifft(H_LS) mode)
      OFDM_TRY(rx_chain_task5_run(pl, b.rx, nf, (uint8_t*)dec, nullptr, nullptr, nullptr, nullptr, nullptr, rxflags, inv_snr));
    }
    const int64_t frame = at - p * FR;                           // the chunk's first frame among the point's F repeats frames
    if (rows) {
      hipLaunchKernelGGL(payload_join_kernel, dim3(payload_grid(nf * s.frame_words)), dim3(PAY_THREADS), 0, stream,
                         (const uint32_t*)dec, cut, frame, nf, s.frame_words, (int64_t)row_words,
                         (uint32_t*)rows + (size_t)p * R * row_words);
      OFDM_TRY(check_launch("payload_join_kernel"));
    }
    const unsigned frame_blocks = (unsigned)std::min<int64_t>(nf, PAY_MAX_GRID);
    hipLaunchKernelGGL(payload_tally_kernel, dim3(payload_tally_grid(nf, dones ? n_bits : 0)), dim3(PAY_THREADS), 0, stream,
                       (const uint32_t*)dec, (const uint32_t*)b.ref, cut, frame, nf, s.frame_words, frame_blocks, derr + (size_t)p * R,
                       dfe ? (uint32_t*)dfe + (size_t)p * (size_t)FR : nullptr, dones ? (uint32_t*)dones + (size_t)p * (size_t)n_bits : nullptr);
    return check_launch("payload_tally_kernel");
  }));
  if (ddec)                                                      // the staging rows are whole words, the caller's whole bytes
    OFDM_HIP(hipMemcpy2DAsync(ddec, row_bytes, rows, sizeof(uint32_t) * row_words, row_bytes, P * R, hipMemcpyDeviceToDevice, stream));
  return st.finish();
}
