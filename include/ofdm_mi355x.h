/*
 * ofdm_mi355x.h -- C ABI of libofdm_mi355x.so (MI355X / gfx950 native OFDM baseband hot path).
 *
 * Drop-in boundary for the Task 1-5 TX -> channel -> RX path of ladnlav/OFDM-course.
 * The reference has no FFI layer: its boundary is the MATLAB function-call interface
 * (one `function` per .m file).  Each entry point below replaces
 * exactly one reference function and is what a MEX gateway (mex/<name>.cpp, see
 * INTEGRATION.md) binds.  "T5/x.m:a-b" = /root/reference/Task 5/x.m lines a-b.
 *
 * Conventions (all entries):
 *   - arrays are MATLAB column-major; complex data is interleaved (re,im);
 *   - `flags` bit0: OFDM_F64 -> data are double / complex double, else float / complex float;
 *     the kernels compute in that same type (fp64 = parity mode, fp32 = throughput mode);
 *   - `flags` bit1: OFDM_DEVICE -> every *data* pointer is a device (HBM) pointer and the call
 *     is asynchronous on the library stream (ofdm_set_stream); otherwise data pointers are
 *     host pointers, the library stages them through HBM and the call returns synchronised;
 *   - index vectors (`*_carriers`, `pilot_loc`) are HOST int32 arrays holding the reference's
 *     1-based carrier indices; scalar out-params are HOST pointers (a call that returns
 *     scalars synchronises the stream);
 *   - bit vectors are uint8 arrays of 0/1 (one byte per bit), except the fused chain which
 *     uses packed bits (MSB-first inside each byte);
 *   - inputs are never modified; outputs are caller-allocated;
 *   - return value: 0 = ok, <0 = error (invalid argument / shape / HIP failure; text in
 *     ofdm_last_error_string()), >0 = soft condition (documented per function).  Nothing
 *     throws across the boundary.
 */
#ifndef OFDM_MI355X_H
#define OFDM_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDM_F32 0
#define OFDM_F64 1
#define OFDM_HOST 0
#define OFDM_DEVICE 2

/* status codes */
#define OFDM_OK 0
#define OFDM_ERR_ARG (-1)       /* invalid argument / shape (MATLAB would raise an error) */
#define OFDM_ERR_HIP (-2)       /* HIP runtime failure */
#define OFDM_ERR_STATE (-3)     /* library not initialised / no GPU */
#define OFDM_ERR_UNSUPPORTED (-4)
#define OFDM_SOFT_ACF_FALLBACK 1 /* AutoCorrFunction: plateau not found, TgPosition = 65 (T5/AutoCorrFunction.m:21-24) */

/* ---- lifecycle -------------------------------------------------------------------------- */
int ofdm_init(int device_id);                 /* binds the calling process to one GPU          */
int ofdm_shutdown(void);                      /* frees plan / twiddle caches (MEX: mexAtExit)  */
const char* ofdm_last_error_string(void);
int ofdm_set_stream(void* hip_stream);        /* hipStream_t to launch on (NULL = default)     */
int ofdm_synchronize(void);
int ofdm_version(void);

/* ---- constellation / mapping (bit-exact) ------------------------------------------------- */
/* T5/constellation_func.m:4-35.  name in {BPSK,QPSK,8PSK,16QAM} + extensions {64QAM,256QAM}.
 * dict_out: 2^bps complex (host pointer always). */
int ofdm_constellation_func(const char* name, void* dict_out, int* bps_out, int flags);

/* T5/mapping.m:1-25.  bits[n_bits] -> iq[ceil(n_bits/bps)]; *pad_out = -1 when no padding. */
int ofdm_mapping(const uint8_t* bits, int64_t n_bits, const char* constellation,
                 void* iq_out, int* pad_out, int flags);

/* T5/demapping.m:1-25.  iq[n_iq] -> bits_out[n_iq*bps - max(pad,0)] (hard decision, first min). */
int ofdm_demapping(int pad, const void* iq, int64_t n_iq, const char* constellation,
                   uint8_t* bits_out, int flags);

/* ---- scrambler (bit-exact) --------------------------------------------------------------- */
/* T5/Scrambler.m:1-28 / T5/DeScrambler.m:1-28.  reg[15] (host, uint8 0/1) is read AND updated
 * with the final register (second output of the .m function). */
int ofdm_Scrambler(uint8_t* reg15, const uint8_t* seq, int64_t n, uint8_t* out, int flags);
int ofdm_DeScrambler(uint8_t* reg15, const uint8_t* seq, int64_t n, uint8_t* out, int flags);
/* Per-frame batch used by the drivers (register reset to reg15 for every frame,
 * T5/Main_model_Task_5.m:58-69): seq/out are [frame_len x n_frames] column-major. */
int ofdm_Scrambler_frames(const uint8_t* reg15, const uint8_t* seq, int64_t frame_len,
                          int64_t n_frames, uint8_t* out, int flags);
int ofdm_DeScrambler_frames(const uint8_t* reg15, const uint8_t* seq, int64_t frame_len,
                            int64_t n_frames, uint8_t* out, int flags);

/* ---- carriers / OFDM (I)FFT + CP ---------------------------------------------------------- */
/* T5/OFDM_map_carriers.m:2-9.  payload[n_data*n_symb]; pilot_values[n_pilots*n_symb] or a single
 * complex value when pilot_scalar != 0 (T3/Main_model_Task_3.m:59); out[nfft*n_symb]. */
int ofdm_OFDM_map_carriers(const void* payload, int64_t n_symb, int nfft,
                           const int32_t* data_carriers, int n_data,
                           const int32_t* pilot_carriers, int n_pilots,
                           const void* pilot_values, int pilot_scalar, void* out, int flags);
/* T5/get_payload.m:2-4.  x[nfft*n_symb] -> out[n_data*n_symb]. */
int ofdm_get_payload(const void* x, int nfft, int64_t n_symb,
                     const int32_t* data_carriers, int n_data, void* out, int flags);
/* T5/OFDM_modulator.m:2-11.  x[nfft*n_symb] -> y[(nfft+t_guard)*n_symb] (ifft, 1/nfft, CP). */
int ofdm_OFDM_modulator(const void* x, void* y, int nfft, int64_t n_symb, int t_guard, int flags);
/* T5/OFDM_demodulator.m:2-10.  y[(nfft+t_guard)*n_symb] -> x[nfft*n_symb] (strip CP, fft). */
int ofdm_OFDM_demodulator(const void* y, void* x, int nfft, int64_t n_symb, int t_guard, int flags);

/* ---- channel side ------------------------------------------------------------------------ */
/* T5/get_MP_channel_resp.m:2-19.  taps: host double [n_taps x 2] column-major (delay, amplitude)
 * (+ optional imaginary amplitudes taps_im[n_taps], may be NULL).  h_out[max_delay+1] and
 * H_out[nfft] complex, HOST pointers; *h_len_out = max_delay+1. */
int ofdm_get_MP_channel_resp(const double* taps, const double* taps_im, int n_taps, int nfft,
                             void* h_out, int* h_len_out, void* H_out, int flags);
/* conv(x,h.','full')(1:len) -- T5/Main_model_Task_5.m:126-127.  h is a HOST complex array. */
int ofdm_channel_conv(const void* x, int64_t len, const void* h, int h_len, void* y, int flags);
/* Batch of independent streams (one Monte-Carlo frame each, T5/Task5_part2.m:148-152): x/y are
 * [frame_len x n_frames] column-major, every frame starts from silence. */
int ofdm_channel_conv_frames(const void* x, int64_t frame_len, int64_t n_frames, const void* h, int h_len,
                             void* y, int flags);
/* T5/Noise.m:1-12 with a counter-based generator (Philox4x32-10 + Box-Muller, seed/stream):
 * y = x + sqrt(P/snr/2)*(n_re + i n_im).  *n_var_out = sqrt(NoisePower) (Noise.m:11). */
int ofdm_Noise(double snr_db, const void* x, int64_t len, uint64_t seed, uint32_t stream,
               void* y, double* n_var_out, int flags);
/* One Noise() call per frame (power measured per frame, Philox stream = stream0 + frame). */
int ofdm_Noise_frames(double snr_db, const void* x, int64_t frame_len, int64_t n_frames, uint64_t seed,
                      uint32_t stream0, void* y, int flags);
/* The same with frame f at its own snr_db[f] (HOST array): the SNR sweep of T5/Main_model_Task_5.m:305-307 as a batch. */
int ofdm_Noise_frames_snr(const double* snr_db, const void* x, int64_t frame_len, int64_t n_frames, uint64_t seed,
                          uint32_t stream0, void* y, int flags);
/* T5/add_STO.m:1-10 and T5/add_CFO.m:1-8. */
int ofdm_add_STO(const void* y, int64_t len, int64_t n_sto, void* out, int flags);
int ofdm_add_CFO(const void* y, int64_t len, double cfo, int nfft, void* out, int flags);
/* add_STO then add_CFO of a batch of frames y[frame_len x n_frames], frame f with its own n_sto[f] (int64) and cfo[f]
 * (double) -- the per-run draws of T4/Main_model_Task_4.m:101-110; either array may be NULL (stage off).  The arrays
 * live where `flags` says. */
int ofdm_add_STO_CFO_frames(const void* y, int64_t frame_len, int64_t n_frames, const int64_t* n_sto, const double* cfo,
                            int nfft, void* out, int flags);

/* ---- synchronisation --------------------------------------------------------------------- */
/* T5/AutoCorrFunction.m:1-28.  rho_out[len-width-nfft] complex (may be NULL);
 * returns OFDM_SOFT_ACF_FALLBACK when the catch branch (:21-24) is taken. */
int ofdm_AutoCorrFunction(const void* rx, int64_t len, int width_window, int nfft,
                          void* rho_out, int64_t* tg_position_out, double* freq_offset_out, int flags);
/* T5/remove_IFO.m:1-11. */
int ofdm_remove_IFO(const void* rx, int64_t len, int nfft, void* fixed_out, int* ifo_out, int flags);
/* T5/fine_sync.m:1-45 (variant 0) / T4/fine_sync.m:1-60 (variant 1).  pilot_values[n_pilots*n_symb].
 * tau_out / phase_out (HOST, may be NULL) receive the two internal estimates. */
int ofdm_fine_sync(const void* rx, int nfft, int64_t n_symb, const int32_t* pilot_carriers, int n_pilots,
                   const void* pilot_values, int time_desync, int freq_desync, int variant,
                   void* out, double* tau_out, double* phase_out, int flags);

/* ---- channel estimation / equalisation ---------------------------------------------------- */
/* T5/interpolate.m:1-24.  method: 'l'inear or 's'pline.  h[n_pilots] -> out[n_out]. */
int ofdm_interpolate(const void* h, const int32_t* pilot_loc, int n_pilots, int n_out, char method,
                     void* out, int flags);
/* T5/estimate_channel.m:1-9.  all_carriers[n_all] (1-based query points). */
int ofdm_estimate_channel(const void* rx, int nfft, int64_t n_symb, const int32_t* all_carriers, int n_all,
                          const int32_t* pilot_carriers, int n_pilots, const void* pilot_values,
                          void* h_est_out, void* h_pilots_out, int flags);
/* T5/equalize_signal.m:1-8. */
int ofdm_equalize_signal(const void* x, int nfft, int64_t n_symb, const void* h_est, int n_carrier,
                         void* out, int flags);
/* T5/LS_CE.m:1-34 (symbol 1 only).  y[nfft*n_symb], xp[n_pilots*n_symb] -> h_ls[n_carrier]. */
int ofdm_LS_CE(const void* y, int nfft, int64_t n_symb, const void* xp, const int32_t* pilot_loc,
               int n_pilots, int n_carrier, void* h_ls_out, int flags);
/* T5/MMSE_CE.m:1-39.  h[h_len] = CIR guess, snr_db.  The rms delay spread of :19-24 has r2 - r^2 clamped at 0 (all the energy
 * of h in one bin: the exact value is 0, the computed one rounding noise of either sign; MMSE_CE.m takes a complex sqrt there). */
int ofdm_MMSE_CE(const void* y, int nfft, int64_t n_symb, const void* xp, const int32_t* pilot_loc,
                 int n_pilots, int n_carrier, const void* h, int h_len, double snr_db,
                 void* h_mmse_out, int flags);
/* Sensing matrix of T5/Main_model_Task_5.m:182-190 in closed form: s_out[n_pilots x k]. */
int ofdm_sensing_matrix(const int32_t* pilot_carriers, int n_pilots, int nfft, int k, void* s_out, int flags);
/* T5/MP_estimate.m:1-34.  y[n_pilots], s[n_pilots x k]; H_out[nfft], h_out[nfft],
 * picks_out[dominant_taps] (HOST int32, 1-based, may be NULL). */
int ofdm_MP_estimate(const void* y, const void* s, int n_pilots, int k, int nfft, int dominant_taps,
                     void* H_out, void* h_out, int32_t* picks_out, int flags);
/* T5/OMP_estimate.m:1-37.  index_out[dominant_taps] (HOST, 1-based), *n_index_out = picks made. */
int ofdm_OMP_estimate(const void* y, const void* s, int n_pilots, int k, int nfft, int dominant_taps,
                      double snr_db, void* H_out, void* h_out, int32_t* index_out, int* n_index_out, int flags);

/* ---- metrics ----------------------------------------------------------------------------- */
/* T5/BER_func.m:1-7: *n_errors_out = sum(tx != rx) (HOST).  BER = n_errors / n. */
int ofdm_BER_func(const uint8_t* bit_tx, const uint8_t* bit_rx, int64_t n, int64_t* n_errors_out, int flags);
/* T5/MER_func.m:1-26. */
int ofdm_MER_func(const void* iq, int64_t n, const char* constellation, double* mer_db_out, int flags);

/* ---- PAPR study of Task 2 (T2/Main_model_Task_2.m:69-82) ------------------------------------- */
/* T2/calculatePAPR.m:2-11: *papr_db_out = 10 log10(max|x|^2 / mean|x|^2) (HOST scalar). */
int ofdm_calculatePAPR(const void* x, int64_t n, double* papr_db_out, int flags);
/* T2/calculate_window_PAPR.m:2-15: paprs_out[i] = PAPR of x(i : i+Nfft-1), i < n - nfft + 1 (double whatever the
 * input precision; nothing is written when n < nfft).  O(1) per window (sliding maximum + prefix sums), nfft <= 8192. */
int ofdm_calculate_window_PAPR(const void* x, int64_t n, int nfft, double* paprs_out, int flags);
/* T2/calculateCCDF.m:2-6 ([CCDF, x] = ecdf(values); CCDF = 1 - CCDF): sorted distinct values with the smallest one
 * repeated in front, NaN ignored.  Outputs hold up to n + 1 doubles; *n_out (HOST) = entries written. */
int ofdm_calculateCCDF(const double* papr_values, int64_t n, double* papr_ccdf_out, double* ccdf_out, int64_t* n_out, int flags);

/* ---- fused Task-5 RX chain (the benchmark path; everything stays in HBM) -------------------- */
/* Per frame of n_symb symbols (call order of T5/Task5_part2.m:169-193,:272,:279-303 with the
 * sensing matrix of T5/Main_model_Task_5.m:182-190):
 *   OFDM_demodulator -> Y = RX(pilots,1)./pilot -> OMP_estimate -> equalize_signal(1..n_carrier)
 *   -> get_payload -> demapping -> BER_func against ref bits.
 * The plan owns carrier index tables, the pilot column and the sensing matrix on the device. */
typedef struct ofdm_rx_plan ofdm_rx_plan;
int ofdm_rx_plan_create(ofdm_rx_plan** plan_out, int nfft, int t_guard, int n_symb, int n_carrier,
                        const int32_t* pilot_carriers, int n_pilots,
                        const int32_t* data_carriers, int n_data,
                        const void* pilot_values_col /* [n_pilots] complex, HOST */,
                        int k_atoms, int dominant_taps, const char* constellation, int flags);
int ofdm_rx_plan_destroy(ofdm_rx_plan* plan);
/* rx[(nfft+t_guard)*n_symb*n_frames] (DEVICE or HOST per flags);
 * bits_out: packed decided bits, per frame ceil(n_data*n_symb*bps/8)*... see ofdm_rx_plan_frame_bytes;
 * ref_bits (may be NULL): packed reference bits, same layout;
 * errors_out[n_frames] uint32 bit errors per frame (may be NULL when ref_bits is NULL);
 * h_out (may be NULL): [n_carrier x n_frames] OMP estimate; index_out (may be NULL): [dominant_taps x n_frames]
 * 1-based picks, 0 = unused slot. */
/* MMSE mode of a plan: ofdm_rx_chain_task5 then estimates the channel of every frame with
 * MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR) (T5/MMSE_CE.m:1-39, as called per Monte-Carlo run at
 * T5/Task5_part2.m:176-177) instead of OMP_estimate, and index_out is not written.  For a fixed (h, SNR) that
 * estimator is one linear operator on the pilot LS values of symbol 1 (rms delay spread :19-24, Rpp :33-35, the
 * mrdivide of :36 and the spline re-interpolation of :38 folded together); it is built here once, on the host in
 * double, and applied to a whole batch as one complex GEMM (matrix cores in fp32).  h: host array of n_h complex
 * values in the precision of `flags` (OFDM_F32 / OFDM_F64); h = NULL returns the plan to OMP mode.
 * The rms delay spread has r2 - r^2 clamped at 0 (a one-tap h = a pure delay gives tau_rms = 0, never NaN); an all-zero h is refused.
 * Needs 2..512 pilots; the chain call needs the fast-path geometry (Nfft 512..4096). */
int ofdm_rx_plan_set_mmse(ofdm_rx_plan* plan, const void* h, int64_t n_h, double snr_db, int flags);
/* MMSE mode without a supplied channel: per frame H_LS = LS_CE(Y, Xp, pilot_loc, N_carrier), h = ifft(H_LS) (N_carrier points),
 * H = MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, snr_db)   -- T5/Main_model_Task_5.m:178-180, :317-319.
 * snr_db is what ofdm_rx_chain_task5(_ex) uses; the BER sweeps use snr_db[p] of the point instead.
 * enable = 0 returns the plan to OMP mode (as ofdm_rx_plan_set_mmse(h = NULL) does). Pilot limits: those of ofdm_rx_plan_set_mmse.
 * The two MMSE modes exclude each other: setting one clears the other.  index_out is not written.  The rms delay spread of
 * MMSE_CE.m:19-24 is formed per frame from three Hermitian forms on the pilot LS values (built once per plan, summed in double
 * in both precisions, r2 - r^2 clamped at 0), the Np x Np system of :33-36 is solved per frame (Levinson), :38 is the plan's
 * spline operator.  The generic single-kernel entry refuses the mode as it refuses the fixed-h mode. */
int ofdm_rx_plan_set_mmse_ls(ofdm_rx_plan* plan, int enable, double snr_db);
/* Task-4 receiver over a batch of frames, each frame one stream of N_symb guarded symbols (T4/Main_model_Task_4.m:278-347
 * per frame, the plan supplying Nfft, T_guard, N_symb, the carrier sets, the pilot column and the constellation):
 *   if time_desync || freq_desync:  AutoCorrFunction(Rx, T_guard, Nfft)                              (:278)
 *   if time_desync:                 add_STO(Rx, TgPosition); add_STO(., -(Nfft+T_guard))             (:292-294)
 *   if freq_desync:                 add_CFO(., -FreqOffset, Nfft); remove_IFO(., Nfft)               (:301-303)
 *   OFDM_demodulator; fine_sync (Task-4 variant) if either flag                                      (:310-314)
 *   if mp_desync:                   estimate_channel + equalize_signal                               (:318-334)
 *   get_payload; demapping                                                                           (:340-347)
 * bits_out: packed demapped bits per frame (layout of ofdm_rx_chain_task5), after the per-frame DeScrambler of :354-364
 * when the plan has one (ofdm_rx_plan_set_descrambler); errors_out: differences to ref_bits (the scrambled bits without
 * a descrambler, the payload bits with it).
 * tg_position_out / freq_offset_out / ifo_out: the per-frame estimates (0 where a stage is off);
 * status_out: 0 ok, 1 = AutoCorrFunction's catch branch (TgPosition 65, :19-24), -1 = remove_IFO found no line above
 * 0.77 (the script would abort at remove_IFO.m:8; the frame is decoded with IFO = 0), -2 = TgPosition beyond AutoCorr.
 * h_out (optional): H_est(1..N_carrier) per frame.  All arrays live where `flags` says.  At most 65535 frames per call. */
int ofdm_rx_chain_task4(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int time_desync, int freq_desync, int mp_desync,
                        uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out, int64_t* tg_position_out,
                        double* freq_offset_out, int32_t* ifo_out, int32_t* status_out, void* h_out, int flags);
/* ofdm_rx_chain_task4 that also returns the sums of MER_func (T5/MER_func.m:3-25; the MER reported beside the BER at
 * T3/Main_model_Task_3.m:186, T4/Main_model_Task_4.m:374, and the MER(SNR) study of T4:136-200) over each frame's
 * RX_IQ = get_payload(.)(:), the equalised, fine-synced points the demapper decides, taken from index mer_skip on:
 *   mer_sums_out[n_frames][2] (double, where `flags` says) = {sum |ideal|^2, sum |ideal - RX_IQ|^2} with ideal the nearest
 *   constellation point (the demapper's decision), over the 0-based IQ indices mer_skip .. nd * N_symb - 1.
 * MER = 10 log10(sum s1 / sum s2); summed over frames it is MER_func of the frames' RX_IQ concatenated, as a multi-frame
 * run of the reference computes it.  mer_skip = Nfft + T_guard reproduces RX_IQ(Nfft+T_Guard+1:end) of T4:163; it must lie
 * in 0 .. nd * N_symb - 1.  Frames with status -1 or -2 are included, decoded as ofdm_rx_chain_task4 decodes them; a frame
 * whose equaliser is not finite gives NaN sums, as MER_func is NaN on such an RX_IQ.  The
 * per-frame sums are reduced in a fixed order (no atomics): bitwise independent of the batching.  mer_sums_out = NULL is
 * ofdm_rx_chain_task4; every other output is that call's, bit for bit. */
int ofdm_rx_chain_task4_ex(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int time_desync, int freq_desync,
                           int mp_desync, uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out,
                           int64_t* tg_position_out, double* freq_offset_out, int32_t* ifo_out, int32_t* status_out,
                           void* h_out, int64_t mer_skip, double* mer_sums_out /* [n_frames][2] */, int flags);
/* ofdm_rx_chain_task4_ex that also returns a window of each frame's RX_IQ = get_payload(.)(:) -- the constellation the
 * reference's drivers plot: scatterplot(RX_IQ(length(dataCarriers)+1 : 2*length(dataCarriers))) at
 * T3/Main_model_Task_3.m:154 and T4/Main_model_Task_4.m:165, one scatter per SNR point in the fine-sync study of T4:137-203,
 * and, with the three desync flags off, the unsynchronised constellations of the Task-3 figures (CFO / STO / multipath):
 *   iq_out[n_frames][iq_count] (complex in the plan's precision, where `flags` says) = RX_IQ(iq_first .. iq_first + iq_count - 1)
 *   (0-based) of each frame: the equalised point with fine_sync's rotation applied, exactly the value the demapper slices and
 *   MER_func sums, element i = s * nd + (data index) of symbol s.
 * The window may start anywhere, straddle symbol boundaries and end at nd * N_symb; OFDM_ERR_ARG unless 0 <= iq_first,
 * 1 <= iq_count and iq_first + iq_count <= nd * N_symb (checked behind the plan / mer_skip checks of ofdm_rx_chain_task4_ex,
 * before anything is launched).  Frames with status -1 / -2 are captured as they are decoded; a non-finite equaliser gives
 * non-finite values, as the reference's RX_IQ would be.  iq_out = NULL is ofdm_rx_chain_task4_ex (the window is not looked
 * at); every other output is that call's, bit for bit, whether or not iq_out is given. */
int ofdm_rx_chain_task4_iq(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int time_desync, int freq_desync,
                           int mp_desync, uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out,
                           int64_t* tg_position_out, double* freq_offset_out, int32_t* ifo_out, int32_t* status_out,
                           void* h_out, int64_t mer_skip, double* mer_sums_out /* [n_frames][2] */, int64_t iq_first,
                           int64_t iq_count, void* iq_out /* [n_frames][iq_count] */, int flags);
/* Synthetic RX frames of the plan's geometry, generated on the device (no host payload), per frame:
 *   payload (one Philox4x32-10 draw per QAM symbol, stream = frame0 + f)
 *   -> Scrambler with the register reset per frame (T5/Main_model_Task_5.m:55-69; scr_reg15 = HOST uint8[15], NULL = off)
 *   -> mapping (T5/mapping.m) -> OFDM_map_carriers with the plan's pilot column on every symbol -> OFDM_modulator
 *   -> channel stages.  noise_first != 0 is the REFERENCE order (T5/Main_model_Task_5.m:106-127, T4/Main_model_Task_4.m:
 *      94-110,:257-267, T5/Task5_part2.m:134,:152):  Noise(snr_db) -> add_STO -> add_CFO -> conv(x, h) truncated per frame;
 *      noise_first == 0 (the order ofdm_tx_frames has always used):  add_STO -> add_CFO -> conv -> Noise, i.e. the SNR is
 *      set on the channel's output.  h = host array of h_len complex taps in the precision of `flags`, NULL = no channel;
 *      noise_on == 0 = no Noise stage.
 *   STO / CFO per frame (T4/Main_model_Task_4.m:101-110): mode 0 = off, 1 = sto_value / cfo_value for every frame,
 *      2 = drawn per frame from Philox counter (0, 0, frame0 + f, 2): Time_Delay = word0 mod (Nfft + T_guard + 1)
 *      [randi([0, Nfft+T_Guard])], Freq_Shift = (word1 mod 31) + ((word2 + 0.5) 2^-32 - 0.5) [randi([0,30]) + (rand-0.5)].
 * rx_out: [frame_samples x n_frames]; ref_bits_out: the packed PAYLOAD (input) bits [n_frames][frame_bytes] in the layout
 * ofdm_rx_chain_task5 compares against (with the Scrambler on, compare after ofdm_rx_plan_set_descrambler);
 * bits_out (optional): the payload, one byte per bit [n_frames][frame_bits]; sc_ref_bits_out (optional, Scrambler on): the
 * packed SCRAMBLED bits, what the demapper decides; sto_out / cfo_out (optional): the per-frame draws (int64 / double).
 * All outputs live where `flags` says.  Results depend on (seed, frame0 + f) only, not on how frames are batched. */
int ofdm_tx_frames_ex(ofdm_rx_plan* plan, const void* h, int h_len, double snr_db, int noise_on, uint64_t seed,
                      int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, int sto_mode, int64_t sto_value,
                      int cfo_mode, double cfo_value, int noise_first, void* rx_out, uint8_t* ref_bits_out,
                      uint8_t* bits_out, uint8_t* sc_ref_bits_out, int64_t* sto_out, double* cfo_out, int flags);
/* = ofdm_tx_frames_ex without Scrambler / STO / CFO and with noise_first = 0 (conv -> Noise; NOT the order of the
 * reference's drivers, which add the noise before the channel -- use ofdm_tx_frames_ex(noise_first = 1) for that). */
int ofdm_tx_frames(ofdm_rx_plan* plan, const void* h, int h_len, double snr_db, int noise_on, uint64_t seed,
                   int64_t frame0, int64_t n_frames, void* rx_out, uint8_t* ref_bits_out, uint8_t* bits_out, int flags);
/* Reference-order frame generator in three sample passes (T5/Main_model_Task_5.m:50-127, T5/Noise.m:3-10,
 * T5/Task5_part2.m:134,:152): payload -> [Scrambler per frame] -> mapping -> OFDM_map_carriers -> OFDM_modulator
 * -> Noise(snr_db) -> conv(h) truncated per frame.  The same draws as ofdm_tx_frames_ex(noise_first = 1, sto_mode =
 * cfo_mode = 0, noise_on = 1): payload Philox (seed, frame0 + f), noise Philox counter (i, 0, frame0 + f, 0) with the
 * Box-Muller of ofdm_Noise, the noise power from the frame's own mean |x|^2 (Noise.m:3).  No STO / CFO (the Task-5
 * receiver has no synchroniser; ofdm_tx_frames_fused_ex adds them for the Task-4 sweeps).  h: HOST array of h_len
 * complex taps in the precision of `flags`, at most 64 nonzero taps at delays <= 4096 (NULL = no channel); scr_reg15: HOST uint8[15] or NULL.
 * rx_out [frame_samples x n_frames], ref_bits_out (packed payload bits, optional), sc_ref_bits_out (packed scrambled bits,
 * optional, Scrambler on) live where `flags` says.  Results depend on (seed, frame0 + f) only, not on the batching. */
int ofdm_tx_frames_fused(ofdm_rx_plan* plan, const void* h, int h_len, double snr_db, uint64_t seed, int64_t frame0,
                         int64_t n_frames, const uint8_t* scr_reg15, void* rx_out, uint8_t* ref_bits_out,
                         uint8_t* sc_ref_bits_out, int flags);
/* One tile of a BER(SNR) sweep (T3/Main_model_Task_3.m:237-268, T5/Task5_part2.m:134,:148-152): for each point p the frames
 * frame0 .. frame0 + frames_per_point - 1 are generated as ofdm_tx_frames_fused(h, snr_db[p], seeds[p], ...) and decoded by
 * ofdm_rx_chain_task5 on this plan, each frame once.  snr_db[n_points] / seeds[n_points]: HOST arrays.
 * errors_out[n_points] (uint64): bit errors per point; frame_errors_out (optional): [n_points][frames_per_point] uint32;
 * both live where `flags` says.  With scr_reg15 (HOST uint8[15]) the plan must carry a DeScrambler with the same register
 * and the errors count against the payload bits (T3/Main_model_Task_3.m:237-265); without it the plan must not descramble.
 * An MMSE-mode plan is accepted only with n_points == 1 (its operator is built for one SNR); a plan in the
 * ofdm_rx_plan_set_mmse_ls mode with any n_points, point p estimated at snr_db[p].
 * max_frames_per_chunk: 0 = the library's choice (a workspace of about 2 GB); results do not depend on it.
 * With OFDM_DEVICE nothing synchronises the host (apart from a first-call workspace growth) and nothing is reduced on it. */
int ofdm_ber_sweep_task5(ofdm_rx_plan* plan, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                         int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                         int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out, int flags);
/* ofdm_ber_sweep_task5 with the MER of every point (T5/Main_model_Task_5.m:282 beside its BER): each frame is decoded by
 * ofdm_rx_chain_task5_ex, and
 *   mer_sums_out[n_points][2] (double, optional) = the point's {sum s1, sum s2}: MER_func of the point's RX_IQ concatenated,
 *   MER = 10 log10(s1 / s2);
 *   frame_mer_sums_out[n_points][frames_per_point][2] (double, optional): the per-frame sums.
 * The per-point sums are reduced on the device after the last chunk in a fixed order: bitwise independent of
 * max_frames_per_chunk.  Both MER outputs NULL is ofdm_ber_sweep_task5; every other output is that call's, bit for bit.
 * Outputs live where `flags` says; OFDM_DEVICE keeps the no-host-synchronisation rule, MMSE-mode plans the n_points == 1
 * rule of ofdm_ber_sweep_task5. */
int ofdm_ber_sweep_task5_ex(ofdm_rx_plan* plan, const void* h, int h_len, const double* snr_db, const uint64_t* seeds,
                            int64_t n_points, int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                            int64_t max_frames_per_chunk, uint64_t* errors_out, uint32_t* frame_errors_out,
                            double* mer_sums_out /* [n_points][2] */,
                            double* frame_mer_sums_out /* [n_points][frames_per_point][2] */, int flags);
/* ofdm_tx_frames_fused with a channel drawn per frame on one tap-delay line -- the Monte-Carlo realisations of
 * T5/Task5_part2.m:148-155, static taps with random initial phases and unit power standing in for lteFadingChannel:
 *   tap_delay[n_taps] (HOST int32): 0-based sample delays, distinct, each 0 .. 4096;
 *   tap_power[n_taps] (HOST double): linear powers, > 0;  n_taps: 1 .. 64.
 * Draw convention: tap t of frame f uses Philox4x32-10 with counter (t, 0, frame0 + f, 3) and key = seed (counter word 3 is
 * 0 for the noise, 1 for the payload, 2 for STO / CFO); u = (word0 + 0.5) 2^-32;
 *   a_{f,t} = g_t (cospi(2u) + i sinpi(2u)) in double,  g_t = sqrt(tap_power[t] / sum tap_power) (host, double);
 *   rx_f[n] = sum_t a_{f,t} w_f[n - tap_delay[t]], the amplitudes cast to the precision of `flags` as h is.
 * taps_out (optional): [n_frames][n_taps] interleaved complex double, the amplitudes a_{f,t}, where `flags` says.
 * Everything else -- the order payload -> [Scrambler] -> mapping -> OFDM_map_carriers -> OFDM_modulator -> Noise(snr_db) ->
 * conv(h_f) truncated, the payload and noise draws, the outputs -- is ofdm_tx_frames_fused's.  No STO / CFO.  Results depend
 * on (seed, frame0 + f, t) only, never on the batching. */
int ofdm_tx_frames_fading(ofdm_rx_plan* plan, const int32_t* tap_delay, const double* tap_power, int n_taps, double snr_db,
                          uint64_t seed, int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, void* rx_out,
                          uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out, double* taps_out /* [n_frames][n_taps][2] */,
                          int flags);
/* ofdm_ber_sweep_task5_ex over channel realisations: the frames of point p are those of ofdm_tx_frames_fading(tap_delay,
 * tap_power, n_taps, snr_db[p], seeds[p], ...), each with its own channel, and the error of the receiver's channel estimate is
 * summed beside the bit errors (T5/Task5_part2.m:202-205, :309-318).  Per frame
 *   frame_nmse_out[n_points][frames_per_point] (double, optional) = sum_{k=0}^{N_carrier-1} |H_f(k) - Hest_f(k)|^2 with
 *   H_f(k) = sum_t a_{f,t} exp(-2 pi i tap_delay[t] k / Nfft) (= fft(h_f, Nfft) of get_MP_channel_resp, in double) and Hest_f
 *   the h_out of ofdm_rx_chain_task5;
 *   nmse_sums_out[n_points] (double, optional) = the point's sum; its NMSE is nmse_sums / (frames_per_point * N_carrier).
 * Both are summed in a fixed order without atomics (per frame: thread i of 256 takes carriers i, i + 256, ..., a butterfly
 * over each wavefront, the four partials as (p0 + p1) + (p2 + p3); per point the same over the frames, after the last chunk):
 * bitwise independent of max_frames_per_chunk.  A fixed-h MMSE plan is refused (its operator is built for one h); a plan
 * in the ofdm_rx_plan_set_mmse_ls mode is accepted (Hest_f is then that estimator's output).  The other
 * arguments, outputs and rules are those of ofdm_ber_sweep_task5_ex; with both NMSE outputs NULL no estimate is stored. */
int ofdm_ber_sweep_task5_fading(ofdm_rx_plan* plan, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                const double* snr_db, const uint64_t* seeds, int64_t n_points, int64_t frames_per_point,
                                int64_t frame0, const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                                uint32_t* frame_errors_out, double* mer_sums_out /* [n_points][2] */,
                                double* frame_mer_sums_out /* [n_points][frames_per_point][2] */,
                                double* nmse_sums_out /* [n_points] */,
                                double* frame_nmse_out /* [n_points][frames_per_point] */, int flags);
/* ofdm_ber_sweep_task5_fading (all its arguments and outputs stay, each optional as there) or, with the static channel
 * h / h_len at the end of those, ofdm_ber_sweep_task5_ex -- with the constellation of every sweep point as a density
 * accumulated on the device: what the scatter of T5/Main_model_Task_5.m:248-251 becomes when a point is a million frames, over
 * the points MER_func sums at :282.  Exactly one channel is given: n_taps > 0 (tap_delay / tap_power; h must be NULL and h_len
 * 0), or h / h_len with n_taps == 0 (h = NULL: no channel; the NMSE outputs, which need the tap-delay line, must then be NULL).
 * Every decided point with IQ index >= scope_skip, of every frame of point p, is counted once in
 *   density_out[n_points][bins][bins] (uint64, where `flags` says), at [p][row][col] with
 *     scale = bins / (2 * half_width), computed once on the host in double,
 *     col = clamp((int)floor((double(re) + half_width) * scale), 0, bins - 1),
 *     row = the same from im;
 *   the arithmetic is double in both precisions (one function bins on the device and on the host, csrc/scope_plan.hpp); a
 *   point outside +-half_width lands in an edge bin; a point with non-finite re or im is not binned but counted in
 *   density_dropped_out[n_points] (uint64, optional).  Therefore
 *     sum(density[p]) + dropped[p] == frames_per_point * (nd * N_symb - scope_skip).
 * The points are those of ofdm_rx_chain_task5_iq, symbol 1 included, for every estimator of the plan (OMP on the batch or the
 * wide route, fixed-h MMSE with n_points == 1, ofdm_rx_plan_set_mmse_ls) and with a DeScrambler; each frame is decoded on the
 * route of ofdm_rx_chain_task5_ex with the MER sums wanted, whose symbol stage keeps a uint32 grid in its LDS across the
 * frames a workgroup decodes and adds it to density_out with 64-bit atomics.  Counts are integers: bitwise independent of
 * max_frames_per_chunk, of the launch grid and of the order of arrival.  Refused with OFDM_ERR_ARG, behind every check of the
 * entry without a density, in this order and before anything is launched or written: density_out == NULL; bins not 8, 16, 32,
 * 64 or 128; half_width not finite or <= 0; scope_skip outside 0 .. nd * N_symb - 1; the symbol stage's LDS with the grid
 * (4 * bins^2 bytes behind its present regions) beyond that stage's limit (158 KiB for the generic single kernel, 150 KiB for
 * every other stage).
 * The grids are zeroed on the launch stream before the first chunk.  With OFDM_DEVICE the accumulators are the caller's outputs
 * and the call keeps the no-host-synchronisation rule of ofdm_ber_sweep_task5 (first-call growth of a small plan-owned buffer
 * apart, which with OFDM_HOST holds the accumulators until they are copied out).  Every other output is bit for bit what the
 * entry without a density returns with the MER sums wanted; the MER sums themselves are returned only if asked for. */
int ofdm_ber_sweep_task5_scope(ofdm_rx_plan* plan, const int32_t* tap_delay, const double* tap_power, int n_taps,
                               const double* snr_db, const uint64_t* seeds, int64_t n_points, int64_t frames_per_point,
                               int64_t frame0, const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                               uint32_t* frame_errors_out, double* mer_sums_out /* [n_points][2] */,
                               double* frame_mer_sums_out /* [n_points][frames_per_point][2] */,
                               double* nmse_sums_out /* [n_points] */,
                               double* frame_nmse_out /* [n_points][frames_per_point] */, const void* h, int h_len,
                               uint64_t* density_out /* [n_points][bins][bins] */,
                               uint64_t* density_dropped_out /* [n_points], optional */, int bins, double half_width,
                               int64_t scope_skip, int flags);
/* ofdm_tx_frames_fused with the Task-4 impairments, in the reference order (T4/Main_model_Task_4.m:94-110,:257-267,
 * T5/Noise.m:3-10, T5/add_STO.m, T5/add_CFO.m): per frame f of length len = (Nfft + T_guard) * N_symb
 *   w[j] = x[j] + sigma_f n(j)            the noise of Noise.m, Philox counter (j, 0, frame0 + f, 0) of the SOURCE index j
 *   s[m] = w[m + sto_f] (0 outside 0..len-1)   add_STO.m, either sign
 *   z[m] = s[m] exp(2 pi i cfo_f m / Nfft)     add_CFO.m on the shifted stream
 *   rx[n] = sum_t h_t z[n - d_t]               conv truncated
 * still in three sample passes.  sto_mode / cfo_mode: 0 = off, 1 = sto_value / cfo_value for every frame, 2 = drawn per
 * frame from Philox counter (0, 0, frame0 + f, 2) -- the draws of ofdm_tx_frames_ex, which this call reproduces with
 * noise_first = 1 (to rounding).  With both modes 0 the frames are bit-identical to ofdm_tx_frames_fused's.
 * sto_out / cfo_out (optional): the per-frame draws (int64 / double; 0 for a mode-0 stage), where `flags` says.  The other
 * arguments and limits are those of ofdm_tx_frames_fused.  Results depend on (seed, frame0 + f) only. */
int ofdm_tx_frames_fused_ex(ofdm_rx_plan* plan, const void* h, int h_len, double snr_db, uint64_t seed, int64_t frame0,
                            int64_t n_frames, const uint8_t* scr_reg15, int sto_mode, int64_t sto_value, int cfo_mode,
                            double cfo_value, void* rx_out, uint8_t* ref_bits_out, uint8_t* sc_ref_bits_out,
                            int64_t* sto_out, double* cfo_out, int flags);
/* One tile of a BER(SNR) sweep of the Task-4 receiver: for each point p the frames frame0 .. frame0 + frames_per_point - 1
 * are generated as ofdm_tx_frames_fused_ex(h, snr_db[p], seeds[p], sto / cfo modes and values, ...) and decoded by
 * ofdm_rx_chain_task4(time_desync, freq_desync, mp_desync) on this plan, each frame once.
 *   flags (0,0,0), no STO / CFO / h: the BER(SNR) loop of T3/Main_model_Task_3.m:237-268 (Noise -> demodulator -> demap ->
 *   DeScrambler); STO / CFO with the desync flags on: the synchronisation study of T4/Main_model_Task_4.m:99-134.
 * snr_db[n_points] / seeds[n_points]: HOST arrays.  Outputs, where `flags` says:
 *   errors_out[n_points] (uint64): bit errors per point;
 *   status_counts_out[n_points][4] (uint64, optional): frames with rx_chain_task4 status 0, 1, -1, -2;
 *   cfo_abs_err_out[n_points] (double, optional): sum over the point's frames of |FreqOffset + IFO - Freq_Shift|
 *   (T4/Main_model_Task_4.m:113-134), 0 where freq_desync is off; summed in a fixed order, bitwise independent of the chunk;
 *   frame_errors_out[n_points][frames_per_point] (uint32, optional).
 * Scrambler rule of ofdm_ber_sweep_task5: with scr_reg15 the plan must carry a DeScrambler with the same register and the
 * errors count against the payload bits; without it the plan must not descramble.
 * max_frames_per_chunk: 0..65535 (the limit of ofdm_rx_chain_task4); 0 = the library's choice, which budgets the generator
 * workspace and the Task-4 arena together (about 4 GB).  Results do not depend on it.
 * With OFDM_DEVICE nothing is reduced on the host and nothing synchronises it, apart from first-call set-up (the plan's
 * constellation table and workspace growth) and what ofdm_rx_chain_task4 does anyway: its arena growth and the once-per-plan
 * copy of the pilot column. */
int ofdm_ber_sweep_task4(ofdm_rx_plan* plan, const void* h, int h_len, int sto_mode, int64_t sto_value, int cfo_mode,
                         double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                         const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                         const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                         uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out, int flags);
/* ofdm_ber_sweep_task4 with the MER of every point: each frame is decoded by ofdm_rx_chain_task4_ex(mer_skip), and
 *   mer_sums_out[n_points][2] (double, optional) = the point's {sum s1, sum s2}: MER_func of the point's RX_IQ concatenated,
 *   MER = 10 log10(s1 / s2) (T4/Main_model_Task_4.m:163; with STO 12, time_desync = 1, freq_desync = mp_desync = 0 and
 *   mer_skip = Nfft + T_guard a point is the MER(SNR) study of T4:136-200 over frames_per_point realisations);
 *   frame_mer_sums_out[n_points][frames_per_point][2] (double, optional): the per-frame sums.
 * The per-point sums are reduced on the device after the last chunk in a fixed order: bitwise independent of
 * max_frames_per_chunk.  mer_skip: 0 .. nd * N_symb - 1.  Both MER outputs NULL is ofdm_ber_sweep_task4; every other output
 * is that call's, bit for bit.  Outputs live where `flags` says; OFDM_DEVICE keeps the rule of ofdm_ber_sweep_task4. */
int ofdm_ber_sweep_task4_ex(ofdm_rx_plan* plan, const void* h, int h_len, int sto_mode, int64_t sto_value, int cfo_mode,
                            double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                            const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                            const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                            uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                            int64_t mer_skip, double* mer_sums_out /* [n_points][2] */,
                            double* frame_mer_sums_out /* [n_points][frames_per_point][2] */, int flags);
/* ofdm_tx_frames_fading with the Task-4 impairments: a channel drawn per frame (T5/Task5_part2.m:148-155) behind the
 * STO / CFO of T4/Main_model_Task_4.m:94-110,:257-267, in the reference order, per frame f of length len:
 *   w[j] = x[j] + sigma_f n(j)                  Noise.m, the noise of the SOURCE index j
 *   s[m] = w[m + sto_f] (0 outside 0..len-1)    add_STO.m, either sign
 *   z[m] = s[m] exp(2 pi i cfo_f m / Nfft)      add_CFO.m on the shifted stream
 *   rx[n] = sum_t a_{f,t} z[n - tap_delay[t]]   conv with the frame's own taps, truncated
 * still in three sample passes.  tap_delay / tap_power / n_taps, the draw of a_{f,t} (Philox counter (t, 0, frame0 + f, 3)) and
 * taps_out are those of ofdm_tx_frames_fading; sto_mode / cfo_mode / the values, the draw of sto_f / cfo_f (counter
 * (0, 0, frame0 + f, 2)) and sto_out / cfo_out those of ofdm_tx_frames_fused_ex: the two per-frame draws are independent.
 * With both modes 0 the frames are bit-identical to ofdm_tx_frames_fading's.  The other arguments, outputs and limits are
 * those of ofdm_tx_frames_fading.  Results depend on (seed, frame0 + f, t) only, never on the batching. */
int ofdm_tx_frames_fading_ex(ofdm_rx_plan* plan, const int32_t* tap_delay, const double* tap_power, int n_taps, double snr_db,
                             uint64_t seed, int64_t frame0, int64_t n_frames, const uint8_t* scr_reg15, int sto_mode,
                             int64_t sto_value, int cfo_mode, double cfo_value, void* rx_out, uint8_t* ref_bits_out,
                             uint8_t* sc_ref_bits_out, double* taps_out /* [n_frames][n_taps][2] */, int64_t* sto_out,
                             double* cfo_out, int flags);
/* ofdm_ber_sweep_task4_ex with the error of estimate_channel summed beside the bit errors -- the NMSE(SNR) study of
 * T4/Main_model_Task_4.m:205-239 (T5/Task5_part2.m:202-205 per realisation) over frames_per_point realisations.  Per frame
 *   frame_nmse_out[n_points][frames_per_point] (double, optional) = sum_{k=0}^{N_carrier-1} |H(k) - Hest_f(k)|^2 with Hest_f
 *   the h_out of ofdm_rx_chain_task4_ex for that frame and H(k) = sum_t h_t exp(-2 pi i d_t k / Nfft) in double over the
 *   nonzero taps of h (= H_freq(1:N_carrier) of get_MP_channel_resp; 1 without h);
 *   nmse_sums_out[n_points] (double, optional) = the point's sum; its NMSE is nmse_sums / (frames_per_point * N_carrier).
 * Both are summed in the fixed order of ofdm_ber_sweep_task5_fading (no atomics), the points after the last chunk: bitwise
 * independent of max_frames_per_chunk.  Rules:
 *   the NMSE outputs need mp_desync != 0 (otherwise there is no estimate): OFDM_ERR_ARG, the plan stays usable;
 *   frames with status 1, -1 or -2 are included as decoded; a non-finite estimate gives a NaN frame value and a NaN point
 *   sum, as the Task-4 MER sums do;
 *   the value is the reference's plain difference.  With time_desync / freq_desync on, fine_sync takes the channel's mean
 *   group delay and common phase out of X before estimate_channel (T4:313-318), so the difference then contains that ramp
 *   and does not fall to the noise floor: it is reported as it is, not corrected;
 *   the default chunk budget counts the stored estimates.
 * With both NMSE outputs NULL this is ofdm_ber_sweep_task4_ex: every output bit for bit, no estimate stored.  OFDM_DEVICE keeps
 * the no-host-synchronisation rule of ofdm_ber_sweep_task4. */
int ofdm_ber_sweep_task4_nmse(ofdm_rx_plan* plan, const void* h, int h_len, int sto_mode, int64_t sto_value, int cfo_mode,
                              double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                              const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                              const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                              uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                              int64_t mer_skip, double* mer_sums_out /* [n_points][2] */,
                              double* frame_mer_sums_out /* [n_points][frames_per_point][2] */,
                              double* nmse_sums_out /* [n_points] */,
                              double* frame_nmse_out /* [n_points][frames_per_point] */, int flags);
/* ofdm_ber_sweep_task4_nmse over channel realisations: the frames of point p are those of ofdm_tx_frames_fading_ex(tap_delay,
 * tap_power, n_taps, snr_db[p], seeds[p], sto / cfo modes and values, ...), each with its own channel, decoded by
 * ofdm_rx_chain_task4_ex -- the synchroniser (AutoCorrFunction -> remove_IFO -> fine_sync) and the spline equaliser swept over
 * the echo profiles of T5/Task5_part2.m:148-155.  The NMSE outputs are against the frame's own channel,
 *   H_f(k) = sum_t a_{f,t} exp(-2 pi i tap_delay[t] k / Nfft) in double, from the drawn amplitudes;
 * every other argument, output and rule (mp_desync for the NMSE outputs, the statuses included, NaN, the fine_sync ramp, the
 * chunk budget -- which also counts the amplitudes -- and OFDM_DEVICE) is that of ofdm_ber_sweep_task4_nmse. */
int ofdm_ber_sweep_task4_fading(ofdm_rx_plan* plan, const int32_t* tap_delay, const double* tap_power, int n_taps,
                                int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value, int time_desync,
                                int freq_desync, int mp_desync, const double* snr_db, const uint64_t* seeds, int64_t n_points,
                                int64_t frames_per_point, int64_t frame0, const uint8_t* scr_reg15,
                                int64_t max_frames_per_chunk, uint64_t* errors_out, uint64_t* status_counts_out,
                                double* cfo_abs_err_out, uint32_t* frame_errors_out, int64_t mer_skip,
                                double* mer_sums_out /* [n_points][2] */,
                                double* frame_mer_sums_out /* [n_points][frames_per_point][2] */,
                                double* nmse_sums_out /* [n_points] */,
                                double* frame_nmse_out /* [n_points][frames_per_point] */, int flags);
/* ofdm_ber_sweep_task4_nmse (static channel; all its arguments and outputs stay, each optional as there) with the
 * constellation of every sweep point as a density accumulated on the device -- what the scatter per SNR point of
 * T4/Main_model_Task_4.m:137-203 (:165) becomes when a point is a million frames: every decided point with IQ index >=
 * scope_skip, of every frame of point p, is counted once in
 *   density_out[n_points][bins][bins] (uint64, where `flags` says), at [p][row][col] with
 *     scale = bins / (2 * half_width), computed once on the host in double,
 *     col = clamp((int)floor((double(re) + half_width) * scale), 0, bins - 1),
 *     row = the same from im;
 *   the arithmetic is double in both precisions (one function bins on the device and on the host, csrc/scope_plan.hpp); a
 *   point outside +-half_width lands in an edge bin; a point with non-finite re or im is not binned but counted in
 *   density_dropped_out[n_points] (uint64, optional).  Therefore
 *     sum(density[p]) + dropped[p] == frames_per_point * (nd * N_symb - scope_skip).
 * The points are those of ofdm_rx_chain_task4_iq (RX_IQ = get_payload(.)(:), fine_sync's rotation applied; frames with
 * status -1 / -2 as decoded).  scope_skip = Nfft + T_guard is RX_IQ(Nfft+T_Guard+1:end), the span of the study's MER (T4:163).
 * Counts are integers summed with atomics: bitwise independent of max_frames_per_chunk, of the launch grid and of the order of
 * arrival.  Refused with OFDM_ERR_ARG, behind every check of ofdm_ber_sweep_task4_nmse, in this order and before anything is
 * launched or written: density_out == NULL (ofdm_ber_sweep_task4_nmse is the call without it); bins not 8, 16, 32, 64 or 128;
 * half_width not finite or <= 0; scope_skip outside 0 .. nd * N_symb - 1; the equalise / demap stage's LDS with the grid
 * (4 * bins^2 bytes behind its present regions) beyond the 150 KiB every stage is held to.
 * The grids are zeroed on the launch stream before the first chunk.  With OFDM_DEVICE the accumulators are the caller's outputs
 * and the call keeps the no-host-synchronisation rule of ofdm_ber_sweep_task4 (first-call growth of a small plan-owned buffer
 * apart, which with OFDM_HOST holds the accumulators until they are copied out).  Every other output is
 * ofdm_ber_sweep_task4_nmse's, bit for bit. */
int ofdm_ber_sweep_task4_scope(ofdm_rx_plan* plan, const void* h, int h_len, int sto_mode, int64_t sto_value, int cfo_mode,
                               double cfo_value, int time_desync, int freq_desync, int mp_desync, const double* snr_db,
                               const uint64_t* seeds, int64_t n_points, int64_t frames_per_point, int64_t frame0,
                               const uint8_t* scr_reg15, int64_t max_frames_per_chunk, uint64_t* errors_out,
                               uint64_t* status_counts_out, double* cfo_abs_err_out, uint32_t* frame_errors_out,
                               int64_t mer_skip, double* mer_sums_out /* [n_points][2] */,
                               double* frame_mer_sums_out /* [n_points][frames_per_point][2] */,
                               double* nmse_sums_out /* [n_points] */,
                               double* frame_nmse_out /* [n_points][frames_per_point] */,
                               uint64_t* density_out /* [n_points][bins][bins] */,
                               uint64_t* density_dropped_out /* [n_points], optional */, int bins, double half_width,
                               int64_t scope_skip, int flags);
/* Per-frame DeScrambler inside ofdm_rx_chain_task5 / ofdm_rx_chain_task4 (T5/DeScrambler.m:1-16 with
 * the register reset for every frame, T5/Main_model_Task_5.m:257-274, T4/Main_model_Task_4.m:354-364): the demapped bits
 * of a frame go through d[i] = s[i] ^ s[i-13] ^ s[i-14], s[-m] = reg15[m-1], before they are written to bits_out and
 * compared with ref_bits (which then hold the TX's INPUT bits): inside the pack stage of the wave-per-frame symbol kernel
 * (the metric geometry), as one more pass over the packed words on every other path.  ofdm_task5_part2_tile refuses a plan
 * with a DeScrambler (the study runs unscrambled, T5/Task5_part2.m:104-114).  reg15: HOST uint8[15]; NULL = off. */
int ofdm_rx_plan_set_descrambler(ofdm_rx_plan* plan, const uint8_t* reg15);
int64_t ofdm_rx_plan_frame_bytes(const ofdm_rx_plan* plan);   /* packed bytes per frame (4-byte multiple) */
/* One tile of the Monte-Carlo study of T5/Task5_part2.m:148-205, :269-304: n_frames channel realisations jj of the plan's
 * pilot scenario kk, all four estimators on every realisation, nothing but sums returned.
 *   tx_noised[(nfft+t_guard)*n_symb]: the scenario's noisy TX stream (:130-134; DEVICE or HOST per flags);
 *   tap_delay[n_frames][n_ch_taps] (0-based sample delays), tap_amp[n_frames][n_ch_taps] (interleaved complex double):
 *   the realisation's channel (what :150-155 hand to conv, :160-166) -- HOST arrays;
 *   ref_bits: the scenario's packed payload bits, ONE frame (layout of ofdm_rx_chain_task5; all realisations share the TX).
 * Per realisation: conv + truncate, OFDM_demodulator, LS_CE (:174), MMSE_CE with h = the true CIR and snr_db (:176-177),
 * MP_estimate and OMP_estimate with dominant_taps = the plan's (:192-193; the plan's K = the dictionary's columns),
 * NMSE of each against fft(h) on carriers 1..N_carrier (:202-205), equalize_signal / get_payload / demapping / BER_func
 * for each (:269-304).
 *   nmse_out[4][n_frames] (double), errors_out[4][n_frames] (uint32 bit errors): rows LS, MMSE, MP, OMP.
 * The MP projections S^H * residue run as one real GEMM per iteration on the matrix cores in fp32 when Np is a multiple of
 * 16 (dense dictionaries of random pilot masks, :58-64).  At most 65535 realisations and 64 channel taps per call.
 * The rms delay spread of MMSE_CE.m:19-24 is taken over the taps with delay < N_carrier (h_t(1:N_carrier), :176), r2 - r^2 clamped
 * at 0 (a realisation with one such path: tau_rms = 0); a realisation with no such path (0 / 0 in :22) is refused. */
int ofdm_task5_part2_tile(ofdm_rx_plan* plan, const void* tx_noised, const int32_t* tap_delay, const double* tap_amp,
                          int n_ch_taps, int64_t n_frames, double snr_db, const uint8_t* ref_bits, double* nmse_out,
                          uint32_t* errors_out, int flags);
/* One tile of the MSE(SNR) sweep of T5/Main_model_Task_5.m:303-346: the frames of the tile are its n_points SNR values.
 * Per point i:  Noise(snr_db[i], Tx) (:307; Philox stream stream0 + i, key = seed) -> conv(Rx, h) truncated (:308-309) ->
 * OFDM_demodulator (:311) -> LS_CE (:313) -> MMSE_CE with h = ifft(H_est_LS) and snr_db[i] (:314-315) -> MP_estimate and
 * OMP_estimate on Y = RX(pilotCarriers, 1) ./ pilot column with dominant_taps = the plan's (:328-331; the plan's K = the
 * dictionary's columns, :318-320) -> the four mean squared errors against fft(h) on carriers 1..N_carrier (:334-344).
 *   tx[(nfft+t_guard)*n_symb]: the clean TX stream (DEVICE or HOST per flags); tap_delay[n_ch_taps] (0-based sample delays) /
 *   tap_amp[n_ch_taps] (interleaved complex double): the channel, HOST; snr_db[n_points]: HOST;
 *   mse_out[4][n_points] (double, where `flags` says): rows LS, MMSE, MP, OMP.
 * The plan may have no data carriers (comb = 1, the script as committed: pilots on every carrier).  Everything stays on the
 * device: the 61-point sweep of the script is one call.  At most 65535 points and 64 channel taps per call. */
int ofdm_task5_mse_tile(ofdm_rx_plan* plan, const void* tx, const int32_t* tap_delay, const double* tap_amp, int n_ch_taps,
                        const double* snr_db, int64_t n_points, uint64_t seed, uint32_t stream0, double* mse_out, int flags);
/* The OMP_estimate step of the two tiles above (T5/OMP_estimate.m:7-23, Task5_part2.m:193, Main_model_Task_5.m:331) in batch
 * form: n pilot LS vectors y[n_pilots x n] (column per realisation, the plan's precision, DEVICE or HOST per flags like every
 * other array here) against the plan's dictionary -- K consecutive delays of the Nfft-point DFT on the plan's pilot carriers.
 *   index_out[taps x n] (int32): the picks in pick order, 1-based, 0 = not made (the relative-change stop, :20);
 *   x_out[taps x n] (complex double): the coefficient of each pick after the last refit; a pick repeated later holds 0 and the
 *   later one the value (est_fade_chan(index(i)) = x(i), :31-33);  h_out (optional, [n_carrier x n], the plan's precision):
 *   H = fft(est_fade_chan) on carriers 1..N_carrier (:36).
 * route: 0 = the library's choice -- omp_batch_kernel (csrc/ofdm_chain_fast.hip:138; 16 realisations per workgroup, c0 and the
 * Gram table in LDS) for every shape whose state fits 150 KB of LDS, else omp_wide_kernel (csrc/ofdm_omp_wide.hip; one
 * realisation per workgroup, c0 = S^H Y as a transform of Y scattered onto its carriers, scores in registers, dictionary never
 * read): Nfft 512, 1024, 2048 or 4096, K <= Nfft, taps <= 32, any pilot set -- all Nfft delays on a random pilot mask
 * (Task5_part2.m:58-64, :181-184).  1 / 2 force either kernel; a route that cannot serve the shape (omp_batch_kernel beyond its
 * LDS, the wide kernel at Nfft 8192 or below 512) is OFDM_ERR_ARG, never a fallback.  Both kernels give the same picks and, in
 * double, coefficients equal to rounding.  ofdm_rx_chain_task5 and the BER sweeps take the route of their plan
 * (ofdm_rx_plan_set_omp_route): omp_batch_kernel unless the plan says otherwise.
 * The plan's dense dictionary (n_pilots x K, built by ofdm_rx_plan_create) stays: MP_estimate of the tiles reads it.
 * At most 65535 realisations per call. */
int ofdm_OMP_estimate_batch(ofdm_rx_plan* plan, const void* y, int64_t n, int route, int32_t* index_out, void* x_out,
                            void* h_out, int flags);
/* The OMP stage of ofdm_rx_chain_task5(_ex), ofdm_ber_sweep_task5(_ex) and ofdm_ber_sweep_task5_fading on this plan; route is the
 * OMP_ROUTE_* of ofdm_OMP_estimate_batch (0 auto, 1 batch, 2 wide).  A new plan is in 1 (batch): omp_batch_kernel, or the fused
 * symbol-1 + OMP launch where the plan takes it, and its refusal of a state beyond 150 KB of LDS ("OMP stage needs ...").
 *   0 (auto): exactly that route, bit for bit, wherever omp_batch_kernel's state fits; else the three-launch receiver with
 *             omp_wide_kernel in the middle -- K = Nfft on a random pilot mask at Nfft 4096, at Nfft 2048 in double
 *             (Task5_part2.m:58-64, :181-184).
 *   2 (wide): always rx_pilot_kernel (or the split form's pilot stage) -> omp_wide_kernel -> the plan's symbol stage, also on a
 *             plan that would take the fused launch.
 * A shape the chosen kernel cannot serve (the wide kernel at Nfft 8192 or below 512; 2 on a plan of the generic single-kernel
 * entry, which runs its own pursuit: Nfft < 512, a pilot outside 1..N_carrier) makes the receiver call OFDM_ERR_ARG with the
 * reason, before anything is launched; it is never a fallback.  The MMSE modes have no OMP stage and ignore the route.
 * ofdm_rx_plan_get_omp_route: *route_out = the setting, *last_out = the kernel the stage ran in the last receiver call (1 batch --
 * the fused launch included --, 2 wide, 0 none: MMSE mode or the generic entry); either pointer may be NULL. */
int ofdm_rx_plan_set_omp_route(ofdm_rx_plan* plan, int route);
int ofdm_rx_plan_get_omp_route(const ofdm_rx_plan* plan, int* route_out, int* last_out);
/* Measurement aid: with timing enabled every ofdm_rx_chain_task5 call brackets its launches with HIP
 * events on the launch stream; ms3 = {symbol-1 kernel, OMP kernel, symbols kernel} of the last call
 * (comb pilot layouts run the first two as one launch and report {symbol-1 + OMP kernel, 0, symbols
 * kernel}; the generic single-kernel path reports {0, 0, total}). */
int ofdm_rx_plan_set_timing(ofdm_rx_plan* plan, int enable);
int ofdm_rx_plan_last_kernel_ms(ofdm_rx_plan* plan, float* ms3);
/* The same for ofdm_rx_chain_task4: ms5 = {AutoCorrFunction stage, remove_IFO stage, OFDM_demodulator, fine_sync +
 * estimate_channel, equalise + demap (+ DeScrambler)} of the last call (T4/Main_model_Task_4.m:278, :301-303, :308-310,
 * :313-318, :334-364). */
int ofdm_rx_plan_last_task4_ms(ofdm_rx_plan* plan, float* ms5);
int ofdm_rx_chain_task5(ofdm_rx_plan* plan, const void* rx, int64_t n_frames,
                        uint8_t* bits_out, const uint8_t* ref_bits, uint32_t* errors_out,
                        void* h_out, int32_t* index_out, int flags);
/* ofdm_rx_chain_task5 that also returns the sums of MER_func (T5/MER_func.m:3-25; T5/Main_model_Task_5.m:282 reports
 * MER_func(RX_IQ, Constellation) beside the BER) over each frame's whole RX_IQ = get_payload(equalize_signal(.))(:), the
 * equalised points of every data carrier and symbol, symbol 1 included:
 *   mer_sums_out[n_frames][2] (double, where `flags` says) = {sum |ideal|^2, sum |ideal - RX_IQ|^2} with ideal the
 *   constellation point of the demapper's decision, over the 0-based IQ indices 0 .. nd * N_symb - 1.
 * MER = 10 log10(s1 / s2); summed over frames it is MER_func of the frames' RX_IQ concatenated.  A frame whose equaliser is
 * not finite gives NaN sums, as MER_func is NaN on such an RX_IQ.  The sums are taken inside the symbol-stage kernels and
 * reduced per frame in a fixed order (no atomics): bitwise independent of the batching.  With a DeScrambler the wave-per-frame
 * path descrambles in a separate pass when MER is asked for; bits and errors are the same.  mer_sums_out = NULL is
 * ofdm_rx_chain_task5; every other output is that call's, bit for bit. */
int ofdm_rx_chain_task5_ex(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, uint8_t* bits_out, const uint8_t* ref_bits,
                           uint32_t* errors_out, void* h_out, int32_t* index_out, double* mer_sums_out /* [n_frames][2] */,
                           int flags);
/* ofdm_rx_chain_task5_ex that also returns a window of each frame's RX_IQ = get_payload(equalize_signal(.))(:) -- the points
 * the reference looks at at T5/Main_model_Task_5.m:248-251 (RX_IQ = get_payload(...)(:), scatterplot(RX_IQ(nd+1 : nd+332))) and
 * sums in MER_func at :282:
 *   iq_out[n_frames][iq_count] (complex in the plan's precision, where `flags` says) = RX_IQ(iq_first .. iq_first + iq_count - 1)
 *   (0-based) of each frame: the equalised point, exactly the value the demapper slices and MER_func sums, element
 *   i = s * nd + (data index) of symbol s, symbol 1 included.
 * The window may start anywhere, straddle symbol boundaries and end at nd * N_symb; OFDM_ERR_ARG unless 0 <= iq_first,
 * 1 <= iq_count and iq_first + iq_count <= nd * N_symb (checked behind every check and route refusal of ofdm_rx_chain_task5_ex,
 * before anything is launched).  A non-finite equaliser gives non-finite values, as the reference's RX_IQ would be.  With a
 * DeScrambler the captured points are the same: the capture sits in front of the demapper.  The call takes the route of
 * ofdm_rx_chain_task5_ex with the MER sums wanted (the symbol stage runs the capture variant of its MER build); mer_sums_out is
 * still optional.  iq_out = NULL is ofdm_rx_chain_task5_ex (the window is not looked at); every other output is bit for bit
 * what ofdm_rx_chain_task5_ex with mer_sums_out given returns. */
int ofdm_rx_chain_task5_iq(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, uint8_t* bits_out, const uint8_t* ref_bits,
                           uint32_t* errors_out, void* h_out, int32_t* index_out, double* mer_sums_out /* [n_frames][2] */,
                           int64_t iq_first, int64_t iq_count, void* iq_out /* [n_frames][iq_count] */, int flags);
/* The PAPR / CCDF study of T2/Main_model_Task_2.m:69-97 over n_signals signals as one device-resident call.  A signal is
 * frames_per_signal consecutive frames of the plan's geometry, concatenated (T2:64-68): payload -> [Scrambler per frame, register
 * reset, T2:36-51] -> mapping -> OFDM_map_carriers -> OFDM_modulator (T2:53-68) -- the bit and symbol stages of
 * ofdm_tx_frames_fused, no Noise and no channel.  Frame g of the call draws its payload from Philox stream frame0 + g, key `seed`,
 * as the generator does; payload_bits, when given, replace the draw.  Every window of `window` samples of every signal
 * (calculate_window_PAPR.m:8-14; windows never cross a signal's end) is counted by its value v = 10 log10(max |x|^2 / mean |x|^2)
 * (calculatePAPR.m:4-10):
 *   hist_out[n_bins]: bin floor((v - lo_db) * n_bins / (hi_db - lo_db)) for lo_db <= v < hi_db;
 *   tails_out[3]: v < lo_db; v >= hi_db (+Inf included); NaN (the 0 / 0 of an all-zero window) -- the curves of
 *   calculateCCDF.m:2-6 (T2:79,:82) follow from the counts;
 *   signal_out[n_signals][2] (optional): max |x|^2 and sum |x|^2 of each signal, calculatePAPR's two figures (T2:72-73);
 *   tx_out (optional, the plan's precision): the signals themselves, frame after frame.
 * The outputs are overwritten, not accumulated: sum(hist) + sum(tails) = n_signals * (frames_per_signal * frame_samples - window
 * + 1).  window: a power of two, 256 .. 8192, at most the signal's length; n_bins 1 .. 4096; lo_db < hi_db, finite.  The signals
 * are generated in chunks of whole signals in the plan-owned workspace (max_frames_per_chunk > 0 caps the frames of a chunk,
 * rounded down to whole signals, at least one); counts are integers, the maximum is order-free and the sums are taken in index
 * order, so no output depends on the chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of
 * the workspace.  hist_out, tails_out, signal_out, tx_out and payload_bits live where `flags` says. */
int ofdm_papr_study(ofdm_rx_plan* plan, uint64_t seed, int64_t frame0, int64_t n_signals, int frames_per_signal,
                    const uint8_t* scr_reg15,          /* HOST uint8[15] or NULL */
                    const uint8_t* payload_bits,       /* optional: [n_signals*frames_per_signal][frame_bits], one byte per bit, where flags says */
                    int window, int n_bins, double lo_db, double hi_db, int64_t max_frames_per_chunk,
                    uint64_t* hist_out,                /* [n_bins] */
                    uint64_t* tails_out,               /* [3]: below lo, at or above hi, NaN */
                    double* signal_out,                /* optional [n_signals][2]: max |x|^2, sum |x|^2 */
                    void* tx_out,                      /* optional [frame_samples x frames]: the signals themselves */
                    int flags);
/* The amplitude spectrum of received frames, the second picture of every impairment in the reference's reports:
 * abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard))) (T3/Main_model_Task_3.m:138, T5/Main_model_Task_5.m:131), the useful part of
 * symbol 2 (T4/Main_model_Task_4.m:268) and, on a clean stream, abs(RX_OFDM_mapped_carriers(:,1)) (T1/Main_model.m:77).
 * rx: [frame_samples x n_frames] complex in the plan's precision, where `flags` says.  Window w = 0 .. n_windows - 1 of frame f is
 * its samples first + w (Nfft + T_guard) .. + Nfft - 1 (0-based); S = fft(window), forward and unscaled like MATLAB's fft, in the
 * plan's precision (the workgroup transform of csrc/fft_core.hpp):
 *   amp_out[n_frames][n_windows][Nfft] (real, the plan's precision) = |S(k)|, the reference's plot;
 *   power_out[n_frames][Nfft] (double) = sum_w (re^2 + im^2), re and im widened to double before squaring, summed in window order.
 * first = T_guard, n_windows = 1 is the line of T3:138; first = T_guard + s (Nfft + T_guard) the useful part of symbol s + 1.  The
 * window may start anywhere (an odd sample, 0, the last start that fits) and straddle a symbol boundary and a cyclic prefix.
 * OFDM_ERR_ARG, before anything is launched or written, in this order: plan or rx missing; the plan (device: OFDM_ERR_STATE;
 * precision flag; data carriers; pilots in band; Nfft 64 .. 8192); n_frames 0 .. 2^31 - 1; first >= 0; n_windows >= 1; the last
 * window ends at or before frame_samples; amp_out or power_out is given (each is optional).  A non-finite sample gives non-finite
 * rows.  amp_out and power_out live where `flags` says. */
int ofdm_rx_spectrum(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int64_t first, int64_t n_windows,
                     void* amp_out,                    /* optional [n_frames][n_windows][Nfft], real */
                     double* power_out,                /* optional [n_frames][Nfft] */
                     int flags);
/* The averaged periodogram of a sweep as one device-resident call: for every point p the frames frame0 .. frame0 +
 * frames_per_point - 1 of ofdm_tx_frames_fused_ex(h, h_len, snr_db[p], seeds[p], scr_reg15, sto_mode, sto_value, cfo_mode,
 * cfo_value) -- or, with tap_delay / tap_power / n_taps in place of h, of ofdm_tx_frames_fading_ex --, bit for bit, and of each frame
 * the power row of ofdm_rx_spectrum(first, n_windows).  No receiver runs.  (T3/Main_model_Task_3.m:138,:155: the spectra of the
 * report's figures, over as many frames as a sweep point has.)
 *   power_sums_out[n_points][Nfft] (double): the point's power rows summed in frame order, ((0 + P_0) + P_1) + ..;
 *   power_peak_out[n_points][Nfft] (double, optional): the maximum (fmax) over the point's frames and windows of re^2 + im^2;
 *   frame_power_out[n_points][frames_per_point][Nfft] (double, optional): the power rows themselves.
 * The outputs are overwritten.  The frames are generated in chunks of one point's frames in the plan-owned workspace, budgeted with
 * the chunk's power rows beside it (max_frames_per_chunk > 0 caps the frames of a chunk); the sums are taken by one thread per bin in
 * frame order and the maximum is order-free (no atomics on doubles), so every output is bitwise independent of the chunking.  With
 * OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the workspace.  OFDM_ERR_ARG, before anything is
 * launched or written, in this order: plan missing, a negative n_points, frames_per_point or max_frames_per_chunk; snr_db / seeds;
 * too many points; the plan (as above, with the streams of one point); sto_mode / cfo_mode; register entries; h and taps together;
 * the channel (as the generator refuses it); first >= 0; n_windows >= 1; the last window ends at or before frame_samples;
 * power_sums_out is given.  The outputs live where `flags` says. */
int ofdm_spectrum_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                        const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                        int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                        const uint8_t* scr_reg15,      /* HOST uint8[15] or NULL */
                        const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                        int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                        int64_t first, int64_t n_windows,
                        double* power_sums_out,        /* [n_points][Nfft] */
                        double* power_peak_out,        /* optional [n_points][Nfft] */
                        double* frame_power_out,       /* optional [n_points][frames_per_point][Nfft] */
                        int flags);
/* The coarse synchroniser's curve for a batch of frames: plot(abs(AutoCorr)) of T4/Main_model_Task_4.m:282-287 (figures 6-10 of the
 * Task-4 report: WidthWindow 1, T_Guard / 2, T_Guard, Nfft), AutoCorr = AutoCorrFunction(frame, width_window, Nfft)
 * (T4/AutoCorrFunction.m:3-7), with the function's TgPosition (:10-24) and FreqOffset (:27) per frame.
 * rx: [frame_samples x n_frames] complex in the plan's precision, where `flags` says.  n_out = frame_samples - width_window - Nfft
 * lags per frame (:3); the call at T4:278 uses width_window = T_guard.  Per frame, every output optional but one:
 *   amp_out[n_frames][n_out] (real, the plan's precision) = |rho(n)|: sqrt(re^2 + im^2) formed in double from the stored rho, as the
 *     search's threshold test forms it, then rounded to the plan's precision;
 *   rho_out[n_frames][n_out] (complex, the plan's precision): AutoCorr itself, bit for bit that of ofdm_AutoCorrFunction on the frame
 *     (the same tiles of the same prefix sums); a window of zeros stays 0 / 0 = NaN;
 *   tg_position_out[n_frames] (1-based), status_out[n_frames]: 0, or 1 = the catch branch of :21-24 with TgPosition 65;
 *   freq_offset_out[n_frames] = -angle(AutoCorr(TgPosition)) / (2 pi); NaN where the curve has no lag 65 to fall back to (the
 *     reference's index error at :27, still status 1).
 * One workgroup per frame (sync_capture_kernel, csrc/ofdm_sync_study.hip); nothing is fetched to the host beyond the outputs.
 * OFDM_ERR_ARG, before anything is launched or written, in this order: plan or rx missing; the plan (device: OFDM_ERR_STATE;
 * precision flag; data carriers; pilots in band; Nfft 64 .. 8192); n_frames 0 .. 2^31 - 1; width_window 1 .. 1024; n_out >= 1; an
 * output is given.  The outputs live where `flags` says. */
int ofdm_rx_acf(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int64_t width_window,
                void* amp_out,                         /* optional [n_frames][n_out], real */
                void* rho_out,                         /* optional [n_frames][n_out], complex */
                int64_t* tg_position_out,              /* optional [n_frames] */
                int32_t* status_out,                   /* optional [n_frames] */
                double* freq_offset_out,               /* optional [n_frames] */
                int flags);
/* The coarse-sync study of a sweep as one device-resident call: the mean ACF behind figures 6-10 of the Task-4 report over as many
 * noisy frames as a point has, where TgPosition falls, and the fractional frequency-offset error over SNR of
 * T4/Main_model_Task_4.m:113-135 (figure 13a).  For every point p the frames frame0 .. frame0 + frames_per_point - 1 of
 * ofdm_tx_frames_fused_ex(h, h_len, snr_db[p], seeds[p], scr_reg15, sto_mode, sto_value, cfo_mode, cfo_value) -- or, with tap_delay /
 * tap_power / n_taps in place of h, of ofdm_tx_frames_fading_ex --, bit for bit, and of each frame the outputs of
 * ofdm_rx_acf(width_window).  The frames never leave the device and no receiver runs behind the autocorrelation; the integer
 * frequency offset is out of scope (remove_IFO needs the derotated stream and a transform; the cfo_abs_err of
 * ofdm_ber_sweep_task4 covers FreqOffset + IFO - Freq_Shift).  n_out = frame_samples - width_window - Nfft.
 *   acf_sums_out[n_points][n_out] (double): the frames' amp rows, widened to double, summed per lag in frame order,
 *     ((0 + a_0) + a_1) + .., a value that is not finite (the zero tail add_STO leaves: 0 / 0) left out and counted in
 *   acf_dropped_out[n_points][n_out] (optional): for every lag, frames added + dropped = frames_per_point;
 *   acf_peak_out[n_points][n_out] (double, optional): fmax over the frames (0 where no frame has a number);
 *   tg_hist_out[n_points][n_out] (optional): frames by TgPosition - 1; the catch branch's 65 lands in bin 64, and where n_out <= 64
 *     such a frame is counted in fallback_out alone;
 *   fallback_out[n_points] (optional): frames that took the catch branch;
 *   phase_hist_out[n_points][Nfft + T_guard] (optional): frames by (TgPosition - 1 + sto) mod (Nfft + T_guard), made non-negative,
 *     sto the frame's own Time_Delay draw (0 when off): add_STO moves every guard interval by -sto, so this histogram is as sharp
 *     with a random delay as without one.  No "true" position is defined here: the timing error is read from the histogram;
 *   ffo_err_out[n_points][2] (double, optional): {sum |e|, sum e^2} in frame order of the wrapped fractional error e = d - rint(d),
 *     d = FreqOffset - (cfo - rint(cfo)), cfo the frame's own Freq_Shift draw (0 when off), ties to even; NaN once a frame's
 *     FreqOffset is NaN;
 *   frame_tg_out / frame_status_out / frame_fo_out[n_points][frames_per_point] (optional): the per-frame scalars.
 * The outputs are overwritten.  The frames are generated in chunks of one point's frames in the plan-owned workspace, budgeted with
 * the chunk's rows beside it (max_frames_per_chunk > 0 caps the frames of a chunk).  The histograms are integers summed with atomics;
 * every double is summed by one thread in frame order, chunk after chunk in stream order, and the maximum is order-free, so every
 * output is bitwise independent of the chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of
 * the workspace.  OFDM_ERR_ARG, before anything is launched or written, in this order: plan missing, a negative n_points,
 * frames_per_point or max_frames_per_chunk; snr_db / seeds; too many points; the plan (as above, with the streams of one point);
 * sto_mode / cfo_mode; register entries; h and taps together; the channel (as the generator refuses it); width_window 1 .. 1024;
 * n_out >= 1; acf_sums_out is given.  The outputs live where `flags` says. */
int ofdm_sync_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                    const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                    int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                    const uint8_t* scr_reg15,          /* HOST uint8[15] or NULL */
                    const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                    int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                    int64_t width_window,
                    double* acf_sums_out,              /* [n_points][n_out] */
                    uint64_t* acf_dropped_out,         /* optional [n_points][n_out] */
                    double* acf_peak_out,              /* optional [n_points][n_out] */
                    uint64_t* tg_hist_out,             /* optional [n_points][n_out] */
                    uint64_t* fallback_out,            /* optional [n_points] */
                    uint64_t* phase_hist_out,          /* optional [n_points][Nfft + T_guard] */
                    double* ffo_err_out,               /* optional [n_points][2] */
                    int64_t* frame_tg_out,             /* optional [n_points][frames_per_point] */
                    int32_t* frame_status_out,         /* optional [n_points][frames_per_point] */
                    double* frame_fo_out,              /* optional [n_points][frames_per_point] */
                    int flags);

/* The fine synchroniser's curve for a batch of demodulated frames: `taus`, the residual-delay estimate of every pair of adjacent
 * pilots of T4/fine_sync.m:10-30 (T5/fine_sync.m:8-16), which figures 18a / 18b of the Task-4 report plot over the carrier number
 * (the commented lines T4/fine_sync.m:10-18), with the mask the report argues for (T4 :32-35, T5 :18-20) and the two estimates.
 * x: [n_frames][N_symb][Nfft] complex in the plan's precision, where `flags` says: per frame the column-major Nfft x N_symb matrix
 * OFDM_demodulator returns and ofdm_fine_sync takes.  The pilots are the plan's (its pilot column on every symbol, T4:28-31).
 * variant: 0 = T5/fine_sync.m, 1 = T4/fine_sync.m.  L = Np * N_symb - 1 for variant 1 when that is >= Np (T4 :8 + :25-30: no trailing
 * 0), else Np * N_symb (the last entry 0).  Per frame, every output optional but one:
 *   taus_out[n_frames][L] (double): angle(q(i+1) conj(q(i))) / (2 pi deltak), q = pilotValues .* conj(rx pilots), before the mask;
 *   keep_out[n_frames][L] (uint8): the mask |taus(i) - taus(i-1)| < 1e-3 (entry 0 false), variant 1 also diff ~= 0 (T4 :33, T5 :18);
 *   tau_out[n_frames] (double): the mean of the kept entries behind the first Np kept ones (T4 :35, T5 :20); NaN = mean([]);
 *   phase_out[n_frames] (double): the mean of the angles qks with |qks| > 1e-3 after the timing derotation by tau when time_desync is
 *     set (T4 :38-52, T5 :23-37); NaN = mean([]);
 *   n_used_out[n_frames] (int32): the denominator of tau; n_phase_out[n_frames] (int32): the denominator of phase.
 * tau and phase are bit for bit what ofdm_fine_sync(.., tau_out, phase_out) returns for the frame with the plan's pilots, the same
 * variant and time_desync, and what the batched Task-4 receiver's fine_sync stage computes (variant 1): one arithmetic, the
 * reductions of csrc/sync_core.hpp with their capture on.  One workgroup per frame (fine_capture_kernel, csrc/ofdm_fine_study.hip).
 * OFDM_ERR_ARG, before anything is launched or written, in this order: plan or x missing; the plan (device: OFDM_ERR_STATE;
 * precision flag; data carriers; pilots in band; Nfft 64 .. 8192); n_frames 0 .. 2^31 - 1; variant 0 / 1; at least two pilots;
 * Np * N_symb < 2^31; an output is given.  The outputs live where `flags` says. */
int ofdm_rx_fine(ofdm_rx_plan* plan, const void* x, int64_t n_frames, int variant, int time_desync,
                 double* taus_out,                     /* optional [n_frames][L] */
                 uint8_t* keep_out,                    /* optional [n_frames][L] */
                 double* tau_out,                      /* optional [n_frames] */
                 double* phase_out,                    /* optional [n_frames] */
                 int32_t* n_used_out,                  /* optional [n_frames] */
                 int32_t* n_phase_out,                 /* optional [n_frames] */
                 int flags);
/* The fine-timing study of a sweep as one device-resident call: the tau curve behind figures 18a / 18b over as many frames as a
 * point has, how many pilot pairs the 1e-3 mask keeps, and the residual-timing error over SNR at the points of
 * T4/Main_model_Task_4.m:137-203.  For every point p the frames frame0 .. frame0 + frames_per_point - 1 of
 * ofdm_tx_frames_fused_ex (or, with taps, ofdm_tx_frames_fading_ex), bit for bit, go through the front end of
 * ofdm_rx_chain_task4(time_desync, freq_desync) exactly as that receiver runs it on the route of csrc/t4_route.hpp --
 * AutoCorrFunction(Rx, T_guard, Nfft), add_STO(TgPosition), add_STO(-(Nfft + T_guard)), with freq_desync add_CFO(-FreqOffset) and
 * remove_IFO, OFDM_demodulator (T4:278-310) -- and of each frame's pilot rows the outputs of ofdm_rx_fine(variant, time_desync).
 * Nothing behind fine_sync's two estimates runs: no equaliser, no demapper, no bit.  L as in ofdm_rx_fine.  Every output optional
 * but one:
 *   tau_curve_sums_out[n_points][L] (double): taus(i) summed over the point's frames in frame order, ((0 + t_0) + t_1) + ..; a value
 *     that is not finite is left out and counted in curve_dropped_out[n_points][L];
 *   keep_counts_out[n_points][L]: the frames whose entry i passed the mask;
 *   tau_hist_out[n_points][bins_n], tau_below_out / tau_above_out / tau_nan_out[n_points]: the frames by their timing error e in
 *     samples, e = tau * Nfft + phi_s + 1, phi = (TgPosition - 1 + Time_Delay) mod (Nfft + T_guard) the guard phase of
 *     ofdm_sync_study, phi_s = phi wrapped into (-(Nfft + T_guard) / 2, (Nfft + T_guard) / 2]: bin floor((e - lo) n / (hi - lo)) on
 *     [bins_lo, bins_hi), below for e < lo, above for e >= hi, nan for tau = NaN; their sum is frames_per_point;
 *   tau_err_out[n_points][2] (double) = {sum |e|, sum e^2} and phase_sums_out[n_points][2] (double) = {sum phase, sum phase^2}, in
 *     frame order over the frames where the value is finite; phase_nan_out[n_points]: the frames whose phase is NaN;
 *   used_sums_out[n_points] = sum n_used;
 *   tg_hist_out[n_points][Nfft + T_guard]: the frames by phi;
 *   frame_tau_out, frame_phase_out (double), frame_n_used_out (int32), frame_tg_out (int64), frame_status_out (int32, the receiver's
 *     status), frame_time_delay_out (int64, the frame's Time_Delay draw) [n_points][frames_per_point]: the per-frame scalars.
 * The outputs are overwritten.  Chunks of one point's frames, budgeted as ofdm_ber_sweep_task4 budgets them with the chunk's rows
 * beside (max_frames_per_chunk > 0 caps the frames of a chunk).  The integer tables are atomics on integers or fixed-order sums;
 * every double is added by one thread in frame order, chunk after chunk in stream order: every output is bitwise independent of
 * the chunking.  OFDM_ERR_ARG, before anything is launched or written, in this order: plan missing, a negative n_points or
 * frames_per_point, max_frames_per_chunk outside 0 .. 65535; snr_db / seeds; too many points; the plan (as above, with the streams
 * of one point); sto_mode / cfo_mode; register entries; h and taps together; the channel (as the generator refuses it); variant;
 * at least two pilots; Np * N_symb < 2^31; time_desync and freq_desync both 0; the receiver's route (its refusals, in its words);
 * bins_n >= 1 and finite bins_lo < bins_hi; an output is given.  The outputs live where `flags` says. */
int ofdm_fine_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                    const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                    int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                    int time_desync, int freq_desync, int variant,
                    const uint8_t* scr_reg15,          /* HOST uint8[15] or NULL */
                    const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                    int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                    int bins_n, double bins_lo, double bins_hi,
                    double* tau_curve_sums_out,        /* optional [n_points][L] */
                    uint64_t* curve_dropped_out,       /* optional [n_points][L] */
                    uint64_t* keep_counts_out,         /* optional [n_points][L] */
                    uint64_t* tau_hist_out,            /* optional [n_points][bins_n] */
                    uint64_t* tau_below_out,           /* optional [n_points] */
                    uint64_t* tau_above_out,           /* optional [n_points] */
                    uint64_t* tau_nan_out,             /* optional [n_points] */
                    double* tau_err_out,               /* optional [n_points][2] */
                    double* phase_sums_out,            /* optional [n_points][2] */
                    uint64_t* phase_nan_out,           /* optional [n_points] */
                    uint64_t* used_sums_out,           /* optional [n_points] */
                    uint64_t* tg_hist_out,             /* optional [n_points][Nfft + T_guard] */
                    double* frame_tau_out,             /* optional [n_points][frames_per_point] */
                    double* frame_phase_out,           /* optional [n_points][frames_per_point] */
                    int32_t* frame_n_used_out,         /* optional [n_points][frames_per_point] */
                    int64_t* frame_tg_out,             /* optional [n_points][frames_per_point] */
                    int32_t* frame_status_out,         /* optional [n_points][frames_per_point] */
                    int64_t* frame_time_delay_out,     /* optional [n_points][frames_per_point] */
                    int flags);

/* The spectrum remove_IFO thresholds, for a batch of frames: abs(fft(rx_signal(Nfft+1 : 2*Nfft))) of T4/remove_IFO.m:5 with
 * IFO = inds(1) - 1 of :6-8, at either of the function's two call sites.
 * rx: [frame_samples x n_frames] complex in the plan's precision, where `flags` says.
 * stage 0: the received frame as it is, AutoCorrFunction beside it (T4/Main_model_Task_4.m:124-125).  stage 1: the stream the
 * receiver hands remove_IFO (T4:278-303): with time_desync add_STO(rx, TgPosition) and add_STO(., -(Nfft + T_guard)) -- the leading
 * zeros are zeros --, then add_CFO(., -FreqOffset), every sample rounded to the plan's precision as the receiver's separate stages
 * round it (t4_raw / t4_rotate, csrc/t4_stream.hpp: the receiver's own bodies).  In both stages TgPosition, FreqOffset and the
 * catch-branch flag come from the receiver's AutoCorrFunction stage (width T_guard), so they are bit for bit the tg_position_out /
 * freq_offset_out of ofdm_rx_chain_task4(time_desync, 1, 0) on the same frames.  Per frame, every output optional but one:
 *   amp_out[n_frames][Nfft] (real, the plan's precision) = |S(k)|: sqrt(re^2 + im^2) formed in double from the spectrum in the
 *     plan's precision (forward, unscaled), as the receiver's threshold test forms it, then rounded to the plan's precision;
 *   ifo_out[n_frames]: the first bin whose |S|, before that last rounding, exceeds 0.77; 0 where no bin does (status -1: the
 *     script stops at inds(1); ofdm_rx_chain_task4 reports -1 there and goes on with an IFO of 0);
 *   status_out[n_frames]: 0; 1 = AutoCorrFunction's catch branch (TgPosition 65); -1 = no bin above 0.77 (it replaces 0 and 1); -2
 *     where the catch branch's lag 65 lies behind the curve (FreqOffset NaN), as in ofdm_rx_chain_task4;
 *   n_above_out[n_frames]: the number of bins whose |S| exceeds 0.77;
 *   tg_position_out[n_frames] (1-based), freq_offset_out[n_frames].
 * In float a bin whose |S| in double lies above 0.77 by less than half a float step counts as above although its amp_out reads
 * 0.76999998.  One transform of Nfft / 8 threads per frame on the workgroup FFT of csrc/fft_core.hpp (ifo_capture_kernel,
 * csrc/ofdm_ifo_study.hip): no complex spectrum and no corrected copy of a frame reaches memory.  OFDM_ERR_ARG, before anything is
 * launched or written, in this order: plan or rx missing; the plan (device: OFDM_ERR_STATE; precision flag; data carriers; pilots
 * in band; Nfft 64 .. 8192); n_frames 0 .. 2^31 - 1; stage 0 / 1; time_desync 0 / 1; a frame shorter than 2 Nfft samples; the
 * receiver's route (its other refusals, in its words: T_guard 1 .. 1024, two pilots); an output is given.  The outputs live where
 * `flags` says. */
int ofdm_rx_ifo(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int stage, int time_desync,
                void* amp_out,                         /* optional [n_frames][Nfft], real */
                int32_t* ifo_out,                      /* optional [n_frames] */
                int32_t* status_out,                   /* optional [n_frames] */
                int32_t* n_above_out,                  /* optional [n_frames] */
                int64_t* tg_position_out,              /* optional [n_frames] */
                double* freq_offset_out,               /* optional [n_frames] */
                int flags);
/* The integer-offset study of a sweep as one device-resident call: figure 13b of the Task-4 report (the loop of
 * T4/Main_model_Task_4.m:113-135, |FreqOffset + e_IFO - Freq_Shift| over SNR) over as many frames as a point has, with the spectrum
 * remove_IFO looks at and where its pick falls.  For every point p the frames frame0 .. frame0 + frames_per_point - 1 of
 * ofdm_tx_frames_fused_ex(h, h_len, snr_db[p], seeds[p], scr_reg15, sto_mode, sto_value, cfo_mode, cfo_value) -- or, with tap_delay /
 * tap_power / n_taps in place of h, of ofdm_tx_frames_fading_ex --, bit for bit, and of each frame the outputs of
 * ofdm_rx_ifo(stage, time_desync).  The frames never leave the device; no demodulator and nothing behind it runs.  Every output
 * optional but one:
 *   spec_sums_out[n_points][Nfft] (double): the frames' amp rows, widened to double, summed per bin in frame order,
 *     ((0 + a_0) + a_1) + ..; a value that is not finite is left out and counted in spec_dropped_out[n_points][Nfft];
 *   above_counts_out[n_points][Nfft]: the frames whose bin exceeds 0.77 (which leakage bins below the true line take the pick);
 *   ifo_hist_out[n_points][Nfft]: the frames with a line, by IFO; no_line_out[n_points]: the frames with status -1; their sum is
 *     frames_per_point;
 *   err_hist_out[n_points][2 err_span + 1], err_below_out / err_above_out[n_points]: the frames with a line by d = IFO -
 *     rint(Freq_Shift), the frame's own draw (0 when off) rounded in double, ties to even: bin d + err_span, below for d < -err_span,
 *     above for d > err_span; their sum is frames_per_point - no_line;  hit_out[n_points]: the frames with d = 0;
 *   cfo_err_out[n_points][2] (double) = {sum |e|, sum e^2} in frame order of e = (FreqOffset + IFO) - Freq_Shift over the frames with
 *     a line and a finite FreqOffset: the y axis of T4:130;
 *   fallback_out[n_points]: the frames whose status is 1;
 *   frame_ifo_out, frame_status_out, frame_n_above_out (int32), frame_tg_out (int64), frame_fo_out (double)
 *     [n_points][frames_per_point]: the per-frame scalars.
 * The outputs are overwritten.  Chunks of one point's frames in the plan-owned workspace, budgeted with the chunk's rows beside it
 * (max_frames_per_chunk > 0 caps the frames of a chunk).  The integer tables are atomics on integers or fixed-order sums; every
 * double is added by one thread in frame order, chunk after chunk in stream order: every output is bitwise independent of the
 * chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the workspace.  OFDM_ERR_ARG, before
 * anything is launched or written, in this order: plan missing, a negative n_points, frames_per_point or max_frames_per_chunk;
 * snr_db / seeds; too many points; the plan (as above, with the streams of one point); sto_mode / cfo_mode; register entries; h and
 * taps together; the channel (as the generator refuses it); stage; time_desync; a frame shorter than 2 Nfft samples; the receiver's
 * route; err_span 1 .. 4096; an output is given.  The outputs live where `flags` says. */
int ofdm_ifo_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                   const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                   int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                   int stage, int time_desync,
                   const uint8_t* scr_reg15,           /* HOST uint8[15] or NULL */
                   const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                   int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                   int64_t err_span,
                   double* spec_sums_out,              /* optional [n_points][Nfft] */
                   uint64_t* spec_dropped_out,         /* optional [n_points][Nfft] */
                   uint64_t* above_counts_out,         /* optional [n_points][Nfft] */
                   uint64_t* ifo_hist_out,             /* optional [n_points][Nfft] */
                   uint64_t* no_line_out,              /* optional [n_points] */
                   uint64_t* err_hist_out,             /* optional [n_points][2 err_span + 1] */
                   uint64_t* err_below_out,            /* optional [n_points] */
                   uint64_t* err_above_out,            /* optional [n_points] */
                   uint64_t* hit_out,                  /* optional [n_points] */
                   double* cfo_err_out,                /* optional [n_points][2] */
                   uint64_t* fallback_out,             /* optional [n_points] */
                   int32_t* frame_ifo_out,             /* optional [n_points][frames_per_point] */
                   int32_t* frame_status_out,          /* optional [n_points][frames_per_point] */
                   int32_t* frame_n_above_out,         /* optional [n_points][frames_per_point] */
                   int64_t* frame_tg_out,              /* optional [n_points][frames_per_point] */
                   double* frame_fo_out,               /* optional [n_points][frames_per_point] */
                   int flags);

/* The channel-estimate capture: both outputs of estimate_channel (T4/estimate_channel.m:6,:8) of a batch of received frames.  The
 * call runs ofdm_rx_chain_task4(time_desync, freq_desync, mp_desync = 1) up to and including estimate_channel -- the front end
 * (AutoCorrFunction, the two add_STO, add_CFO, remove_IFO, the demodulator), fine_sync, the pilot means, the spline -- on the route
 * that receiver takes for these flags; no equaliser, no demapper, no bits.  rx: [n_frames][(Nfft + T_guard) N_symb] complex in the
 * plan's precision.  Every output optional but one:
 *   h_est_out[n_frames][N_carrier] complex, the plan's precision: H_est, bit for bit the h_out of that receiver call;
 *   h_pilots_out[n_frames][Np] complex, the plan's precision: Hest_at_pilots = mean(rx(pilotCarriers,:) ./ pilotValues, 2) on the
 *     fine-synced symbols, the rows the spline operator reads;
 *   tg_position_out, freq_offset_out, ifo_out, status_out[n_frames]: bit for bit those of that receiver call.
 * With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the receiver's arena.  OFDM_ERR_ARG, before
 * anything is launched or written, in this order: plan or rx missing; the plan (device, precision flag, data carriers, pilots in
 * band, Nfft / T_guard); n_frames 0 .. 2^31 - 1; time_desync 0 / 1; freq_desync 0 / 1; fewer than two pilot carriers; the
 * receiver's route; an output is given. */
int ofdm_rx_hest(ofdm_rx_plan* plan, const void* rx, int64_t n_frames, int time_desync, int freq_desync,
                 void* h_est_out,                      /* optional [n_frames][N_carrier] complex */
                 void* h_pilots_out,                   /* optional [n_frames][Np] complex */
                 int64_t* tg_position_out,             /* optional [n_frames] */
                 double* freq_offset_out,              /* optional [n_frames] */
                 int32_t* ifo_out,                     /* optional [n_frames] */
                 int32_t* status_out,                  /* optional [n_frames] */
                 int flags);
/* The channel study of a sweep as one device-resident call: figure 21 of the Task-4 report (T4/Main_model_Task_4.m:318-332: |H_freq|,
 * the stems |Hest_at_pilots|, the dashed |H_est| over the carrier index) over as many frames as a point has, with the error of the
 * estimate per carrier, per pilot and per frame.  For every point p the frames frame0 .. frame0 + frames_per_point - 1 of
 * ofdm_tx_frames_fused_ex(h, h_len, snr_db[p], seeds[p], scr_reg15, sto_mode, sto_value, cfo_mode, cfo_value) -- or, with tap_delay /
 * tap_power / n_taps in place of h, of ofdm_tx_frames_fading_ex --, bit for bit, and of each frame what ofdm_rx_hest(time_desync,
 * freq_desync) returns.  The true channel is H_f(k) = sum_t a_{f,t} e^{-2 pi i d_t k / Nfft} in double on carriers k = 0 ..
 * N_carrier - 1, from the nonzero taps of h or the frame's drawn amplitudes (the expression of the Task-4 sweep's NMSE);
 * |z| = sqrt(re re + im im) in double, the products and the sum rounded one by one.  The frames never leave the device.  Every
 * output optional but one:
 *   est_amp_sums_out, true_amp_sums_out, err_sums_out, amp_err_sums_out[n_points][N_carrier] (double): sum_f |H_est_f(k)|,
 *     sum_f |H_f(k)|, sum_f |H_f(k) - H_est_f(k)|^2, sum_f (|H_est_f(k)| - |H_f(k)|)^2, each added in frame order, ((0 + v_0) + v_1)
 *     + ..; a frame whose H_est_f(k) is not finite (fine_sync's mean of an empty selection) adds nothing to any of the four at
 *     carrier k and is counted in dropped_out[n_points][N_carrier];
 *   pilot_amp_sums_out, pilot_err_sums_out[n_points][Np] (double): sum_f |Hest_at_pilots_f(i)| and sum_f |H_f(pilotCarriers(i)) -
 *     Hest_at_pilots_f(i)|^2, the error before interpolation, with pilot_dropped_out[n_points][Np] as above;
 *   frame_nmse_out[n_points][frames_per_point], nmse_sums_out[n_points] (double): sum_k |H_f(k) - H_est_f(k)|^2 and its sum over the
 *     point's frames, bit for bit those of ofdm_ber_sweep_task4_nmse / _fading with mp_desync = 1 (the same kernels);
 *   frame_amp_nmse_out, amp_nmse_sums_out: the same of (|H_est_f(k)| - |H_f(k)|)^2 -- per frame a stride of 256 per thread, the
 *     butterfly of a wavefront and the four wave partials paired, over the frames the sweeps' fixed-order sum; a frame that is not
 *     finite makes its point NaN, as in nmse_sums_out;
 *   nmse_hist_out[n_points][hist_bins], nmse_below_out, nmse_above_out, nmse_nan_out[n_points]: the frames by 10 log10(frame_nmse /
 *     N_carrier) on hist_bins bins of equal width on [hist_lo_db, hist_hi_db); their sum is frames_per_point.  No logarithm is
 *     taken on the device: the host makes the hist_bins + 1 linear thresholds N_carrier 10^(edge / 10) once, in double, and the
 *     bin is the last threshold not above frame_nmse.  thresholds_out[hist_bins + 1] (double, HOST memory whatever the flags): that
 *     table;
 *   status_counts_out[n_points][4]: the frames with status 0, 1, -1, -2, as ofdm_ber_sweep_task4 reports them.
 * The outputs are overwritten.  Chunks of one point's frames in the plan-owned workspace, budgeted with the receiver's arena and the
 * chunk's rows beside it (max_frames_per_chunk > 0 caps the frames of a chunk).  The integer tables are atomics on integers; every
 * per-carrier double is added by one thread in frame order, chunk after chunk in stream order: every output is bitwise independent
 * of the chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the workspace.  OFDM_ERR_ARG,
 * before anything is launched or written, in this order: plan missing, a negative n_points or frames_per_point,
 * max_frames_per_chunk outside 0 .. 65535; snr_db / seeds; too many points; the plan (as above, with the streams of one point);
 * sto_mode / cfo_mode; register entries; h and taps together; the channel (as the generator refuses it); time_desync; freq_desync;
 * fewer than two pilot carriers; the receiver's route; hist_bins 1 .. 4096 with finite hist_lo_db < hist_hi_db; an output is
 * given.  The outputs but thresholds_out live where `flags` says. */
int ofdm_hest_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                    const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                    int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                    int time_desync, int freq_desync,
                    const uint8_t* scr_reg15,          /* HOST uint8[15] or NULL */
                    const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                    int64_t n_points, int64_t frames_per_point, int64_t frame0, int64_t max_frames_per_chunk,
                    int hist_bins, double hist_lo_db, double hist_hi_db,
                    double* est_amp_sums_out,          /* optional [n_points][N_carrier] */
                    double* true_amp_sums_out,         /* optional [n_points][N_carrier] */
                    double* err_sums_out,              /* optional [n_points][N_carrier] */
                    double* amp_err_sums_out,          /* optional [n_points][N_carrier] */
                    uint64_t* dropped_out,             /* optional [n_points][N_carrier] */
                    double* pilot_amp_sums_out,        /* optional [n_points][Np] */
                    double* pilot_err_sums_out,        /* optional [n_points][Np] */
                    uint64_t* pilot_dropped_out,       /* optional [n_points][Np] */
                    double* nmse_sums_out,             /* optional [n_points] */
                    double* amp_nmse_sums_out,         /* optional [n_points] */
                    double* frame_nmse_out,            /* optional [n_points][frames_per_point] */
                    double* frame_amp_nmse_out,        /* optional [n_points][frames_per_point] */
                    uint64_t* nmse_hist_out,           /* optional [n_points][hist_bins] */
                    uint64_t* nmse_below_out,          /* optional [n_points] */
                    uint64_t* nmse_above_out,          /* optional [n_points] */
                    uint64_t* nmse_nan_out,            /* optional [n_points] */
                    uint64_t* status_counts_out,       /* optional [n_points][4] */
                    double* thresholds_out,            /* optional HOST [hist_bins + 1] */
                    int flags);

/* Error anatomy: where the wrong bits of a batch of frames sit.  bits and ref_bits: [n_frames][ofdm_rx_plan_frame_bytes] packed
 * bits in the layout the receivers write (bits_out) and read (ref_bits): stream bit i of a frame at bit 7 - i % 8 of byte i / 8, the
 * padding of the last word zero or not (it is masked).  Stream bit i has QAM index q = i / bps, label bit r = i % bps (0 = the MSB
 * of the constellation label) and q = s nd + d: OFDM symbol s, data carrier dataCarriers(d + 1) -- the inverse of the receivers'
 * pack stage (csrc/ofdm_chain.hip:323-339).  No receiver runs; of the plan only nd, N_symb, bps and the frame's words are read,
 * so any geometry ofdm_rx_plan_create accepts is accepted.  Every output optional but one, all sums over the n_frames frames:
 *   errors_out[1]: the wrong bits; frames_in_error_out[1]: the frames with at least one;
 *   carrier_out[nd], symbol_out[N_symb], label_out[bps]: the wrong bits per data carrier, per OFDM symbol, per label bit; each
 *     sums to errors_out;
 *   gap_hist_out[gap_bins], gap_above_out[1]: for a frame's errors at stream positions i_0 < i_1 < .. the gaps g_k = i_k - i_(k-1),
 *     within the frame only; gap_hist_out[g - 1] counts the gaps g <= gap_bins, gap_above_out the larger ones; together they sum to
 *     errors_out - frames_in_error_out.  The reference's self-synchronising DeScrambler (T5/DeScrambler.m:8-13: the register is
 *     fed by the received bit, taps on Register(13) and Register(14)) turns one channel error into payload errors at i, i + 13 and
 *     i + 14: peaks at gaps 1 and 13;
 *   frame_errors_out[n_frames] (uint32): the wrong bits of each frame;
 *   map_out[N_symb][nd]: the wrong bits on the time-frequency grid; its sums over s and over d are carrier_out and symbol_out.
 * The outputs are overwritten.  Everything is an integer added in no particular order: every output is bitwise independent of
 * how the frames are spread over launches and workgroups.  With OFDM_DEVICE nothing synchronises the host.  OFDM_ERR_ARG, before
 * anything is launched or written, in this order: plan, bits or ref_bits missing; (OFDM_ERR_STATE) the plan's device; no data
 * carriers; n_frames 0 .. 2^31 - 1; a frame of more than 2^32 - 1 bits; gap_bins 1 .. 1024; an output is given. */
int ofdm_bit_error_profile(ofdm_rx_plan* plan, const uint8_t* bits, const uint8_t* ref_bits, int64_t n_frames, int gap_bins,
                           uint64_t* errors_out,               /* optional [1] */
                           uint64_t* frames_in_error_out,      /* optional [1] */
                           uint64_t* carrier_out,              /* optional [nd] */
                           uint64_t* symbol_out,               /* optional [N_symb] */
                           uint64_t* label_out,                /* optional [bps] */
                           uint64_t* gap_hist_out,             /* optional [gap_bins] */
                           uint64_t* gap_above_out,            /* optional [1] */
                           uint32_t* frame_errors_out,         /* optional [n_frames] */
                           uint64_t* map_out,                  /* optional [N_symb][nd] */
                           int flags);
/* The error anatomy of a sweep as one device-resident call: for every point p the frames frame0 .. frame0 + frames_per_point - 1
 * of ofdm_tx_frames_fused_ex(h, h_len, snr_db[p], seeds[p], scr_reg15, sto_mode, sto_value, cfo_mode, cfo_value) -- or, with
 * tap_delay / tap_power / n_taps in place of h, of ofdm_tx_frames_fading_ex --, bit for bit, decoded as the matching sweep decodes
 * them -- receiver 5: ofdm_rx_chain_task5 as in ofdm_ber_sweep_task5 / _fading (the plan's route, its MMSE, h = ifft(H_LS) and
 * OMP-route modes; sto_mode, cfo_mode, time_desync and freq_desync must be 0 and mp_desync 1); receiver 4: ofdm_rx_chain_task4(
 * time_desync, freq_desync, mp_desync) as in ofdm_ber_sweep_task4 / _fading, the per-point STO / CFO draws as there -- and of the
 * decisions the tables of ofdm_bit_error_profile with a leading n_points.  The frames and the bits never leave the device.
 *   side 0 (payload): what the receiver returns against the payload bits; errors_out is then errors_out of the matching sweep for
 *     the same arguments, bit for bit (T3/Main_model_Task_3.m:237-266, T4/Main_model_Task_4.m:354-366);
 *   side 1 (channel): the decisions in front of the DeScrambler against the scrambled bits (sc_ref_bits_out of the generator), so
 *     that carrier, symbol and label mean what they say; behind the self-synchronising DeScrambler every channel error is three
 *     payload errors.  The receiver runs with the plan's DeScrambler masked for the call; the plan is as it was when the call
 *     returns, errors included.  While a side 1 call runs the plan itself is changed: no other thread may use the plan, and no
 *     other call on it may be issued, until this call has returned (as for every call on a plan, whose workspaces are not
 *     shared either).  Without scr_reg15 the two sides are the same bits.
 * The outputs are overwritten.  Chunks of one point's frames in the plan-owned workspace, budgeted as the matching sweep budgets
 * them with the two bit buffers of a chunk beside them (max_frames_per_chunk > 0 caps the frames of a chunk); every output is
 * bitwise independent of the chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the
 * workspace.  OFDM_ERR_ARG, before anything is launched or written, in this order: receiver 4 / 5; side 0 / 1; h and taps
 * together; receiver 5 with an impairment or a flag ofdm_ber_sweep_task5 does not have; every refusal of the matching sweep in its
 * order and its own words (as "ber_sweep_task5", "ber_sweep_task5_fading", "ber_sweep_task4", "ber_sweep_task4_fading": the
 * generator's channel checks, the Scrambler / DeScrambler rule, the MMSE restrictions, max_frames_per_chunk among them); a frame of
 * more than 2^32 - 1 bits; gap_bins 1 .. 1024; an output is given.  What the receiver's route refuses comes from the first receiver
 * call, in the receiver's words. */
int ofdm_error_study(ofdm_rx_plan* plan, int receiver,        /* 4 | 5 */
                     const void* h, int h_len,                 /* HOST, complex in the plan's precision, or NULL / 0 */
                     const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                     int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                     int time_desync, int freq_desync, int mp_desync,
                     const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                     int64_t n_points, int64_t frames_per_point, int64_t frame0,
                     const uint8_t* scr_reg15,                 /* HOST uint8[15] or NULL */
                     int side,                                 /* 0 payload | 1 channel */
                     int gap_bins, int64_t max_frames_per_chunk,
                     uint64_t* errors_out,                     /* optional [n_points] */
                     uint64_t* frames_in_error_out,            /* optional [n_points] */
                     uint64_t* carrier_out,                    /* optional [n_points][nd] */
                     uint64_t* symbol_out,                     /* optional [n_points][N_symb] */
                     uint64_t* label_out,                      /* optional [n_points][bps] */
                     uint64_t* gap_hist_out,                   /* optional [n_points][gap_bins] */
                     uint64_t* gap_above_out,                  /* optional [n_points] */
                     uint32_t* frame_errors_out,               /* optional [n_points][frames_per_point] */
                     uint64_t* map_out,                        /* optional [n_points][N_symb][nd] */
                     int flags);

/* The estimator comparison of Task 5 as one device-resident call: LS_CE, MMSE_CE, MP_estimate and OMP_estimate on the same
 * received frame of every channel realisation (T5/Task5_part2.m:148-205, :269-304; over SNR T5/Main_model_Task_5.m:303-346).  For
 * every point p the frames frame0 .. frame0 + frames_per_point - 1 of ofdm_tx_frames_fused(h, h_len, snr_db[p], seeds[p]) -- or,
 * with tap_delay / tap_power / n_taps in place of h, of ofdm_tx_frames_fading, a channel realisation per frame --, bit for bit,
 * through the estimator stages of ofdm_task5_part2_tile: OFDM_demodulator, Y = X(pilots, 1) ./ pilotValues(:, 1)
 * (Task5_part2.m:190), the four estimates, and equalize_signal -> get_payload -> demapping -> BER_func against the frame's own
 * payload for each of them (:269-304).  Every [4] below is in the order LS, MMSE, MP, OMP.  The receiver ofdm_rx_chain_task5 and
 * its route are not involved; the study runs unscrambled, as Task5_part2.m:104-114 does.
 *   mmse_mode 0: MMSE_CE with h = ifft(H_est_LS) of the frame at the point's SNR (Main_model_Task_5.m:314-315);
 *   mmse_mode 1: MMSE_CE with the frame's true impulse response (Task5_part2.m:176-177): tau_rms of MMSE_CE.m:19-24 over the taps
 *     with a delay below N_carrier, r2 - r^2 clamped at 0.  A frame with no such tap has no tau_rms: its MMSE estimate is NaN and
 *     the frame is counted in nmse_dropped_out; nothing is refused for what the device drew.
 *   nmse_sums_out[p][e]: the sum over the point's frames, in frame order, of sum_k |fft(h_f, Nfft)(k) - H_e,f(k)|^2 on carriers
 *     1..N_carrier in double (Task5_part2.m:202-205 before the division by N_carrier); a frame whose sum is not finite is left out
 *     and counted in nmse_dropped_out[p][e].  frame_nmse_out keeps every frame's sum, finite or not.
 * The outputs are overwritten.  Chunks of one point's frames: the generator's workspace, the estimator stages' arena and the
 * study's rows on twice the workspace budget (max_frames_per_chunk > 0 caps the frames of a chunk, at most 65535); every output
 * is bitwise independent of the chunking, and a call over frames frame0 .. equals the calls over its parts with the integers
 * added.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of the workspaces.  OFDM_ERR_ARG, before
 * anything is launched or written, in this order: what every study refuses of the generator's arguments and the plan (bad
 * arguments, snr_db / seeds, the plan's device, precision, data carriers, pilots, Nfft, the stream range, h and taps together,
 * the channel); a plan with a DeScrambler; mmse_mode 0 / 1; an output is given; then what ofdm_task5_part2_tile refuses of a
 * plan, in its words (two pilots, the equalise stage's LDS, at most 585 pilots, K >= Np for MP_estimate, the MP stage's LDS).
 * Without errors_out and frame_errors_out no equaliser runs, and H of MP and OMP is the transform of their taps, as in
 * ofdm_task5_mse_tile. */
int ofdm_estimator_study(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                         const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                         const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                         int64_t n_points, int64_t frames_per_point, int64_t frame0,
                         int mmse_mode,                            /* 0 ls | 1 genie */
                         int64_t max_frames_per_chunk,
                         uint64_t* errors_out,                     /* optional [n_points][4] */
                         double* nmse_sums_out,                    /* optional [n_points][4] */
                         uint64_t* nmse_dropped_out,               /* optional [n_points][4] */
                         uint32_t* frame_errors_out,               /* optional [n_points][frames_per_point][4] */
                         double* frame_nmse_out,                   /* optional [n_points][frames_per_point][4] */
                         int flags);

/* The estimator comparison of Task 5 with its two pictures, as one device-resident call: ofdm_estimator_study (the same arguments,
 * the same frames, the same launches; errors_out .. frame_nmse_out are its outputs bit for bit) and, summed over the frames of
 * every point, |H_freq| against |H_est_LS|, |H_est_MMSE|, |H_est_MP|, |H_est_OMP| over the carriers
 * (T5/Main_model_Task_5.m:207-231) and |H_tau| against the delays OMP_estimate picked (:238-242), with the histogram of the
 * frames' error.  Every [4] is in the order LS, MMSE, MP, OMP; K is the plan's dictionary columns, T its dominant_taps.
 *   per carrier: true_amp_sums_out[p][k] = sum_f |H_f(k)| over all frames; est_amp_sums_out[p][e][k] = sum_f |H_e,f(k)|,
 *     err_sums_out = sum_f |H_f(k) - H_e,f(k)|^2, amp_err_sums_out = sum_f (|H_e,f(k)| - |H_f(k)|)^2, in frame order, a frame whose
 *     frame_nmse[f][e] is not finite left out of the three sums of e: the rule and the count of nmse_dropped_out[p][e].
 *     |z| = sqrt(re re + im im) in double, the products and the sum rounded one by one.
 *   the histogram: nmse_hist_out[p][e][b] counts the frames by 10 log10(frame_nmse / N_carrier) on hist_bins bins of equal width
 *     on [hist_lo_db, hist_hi_db), compared against the table of linear thresholds N_carrier 10^(edge / 10) as ofdm_hest_study
 *     does (thresholds_out, HOST [hist_bins + 1] whatever the flags); nmse_below_out / nmse_above_out / nmse_nan_out: the frames
 *     under the grid, over it, and those whose error is not finite (= nmse_dropped_out); the four sum to frames_per_point.
 *   per delay, OMP_estimate only: pick_hist_out[p][k] counts the pick slots whose 0-based delay is k (index - 1 of
 *     OMP_estimate.m:11), tap_amp_sums_out[p][k] = sum |x| of those slots in frame order (a pick repeated later holds 0 in its
 *     earlier slot, so this is sum_f |est_fade_chan_f(k)|); n_picks_hist_out[p][j]: the frames that made j picks (the
 *     relative-change stop of OMP_estimate.m:20); true_tap_amp_sums_out[p][k] = sum_f |a_f,t| of the channel tap with delay
 *     d_t = k < K (the frame's own amplitudes with tap_delay / tap_power, the static channel's otherwise); true_outside_out[p]:
 *     the channel taps with d_t >= K, counted per frame; support_out[p] = {hits, misses, false}: the delays in both the frame's
 *     true support (d_t < K) and its distinct picks, in the true support only, in the picks only, summed over the frames.
 *     picks_out (1-based, 0 = not made) and tap_x_out (complex double whatever the plan's precision) keep every frame's slots.
 *   MP_estimate's delay-domain curve is not offered: the tap workspace holds one pursuit at a time, and the estimator stages turn
 *     MP's taps into H before OMP_estimate overwrites them.  MP's per-carrier rows are there.
 * The outputs are overwritten; every output is bitwise independent of the chunking, and a call over frames frame0 .. equals the
 * calls over its parts with the integers added.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth of
 * the workspaces.  OFDM_ERR_ARG, before anything is launched or written: what ofdm_estimator_study refuses, in its words under
 * the name estimator_profile (up to and including mmse_mode); hist_bins 1 .. 4096 and finite hist_lo_db < hist_hi_db; an output is
 * given; then what ofdm_task5_part2_tile refuses of a plan, in its words. */
int ofdm_estimator_profile(ofdm_rx_plan* plan, const void* h, int h_len, /* HOST, complex in the plan's precision, or NULL / 0 */
                           const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                           const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                           int64_t n_points, int64_t frames_per_point, int64_t frame0,
                           int mmse_mode,                            /* 0 ls | 1 genie */
                           int64_t max_frames_per_chunk,
                           int hist_bins, double hist_lo_db, double hist_hi_db,
                           uint64_t* errors_out,                     /* optional [n_points][4] */
                           double* nmse_sums_out,                    /* optional [n_points][4] */
                           uint64_t* nmse_dropped_out,               /* optional [n_points][4] */
                           uint32_t* frame_errors_out,               /* optional [n_points][frames_per_point][4] */
                           double* frame_nmse_out,                   /* optional [n_points][frames_per_point][4] */
                           double* true_amp_sums_out,                /* optional [n_points][N_carrier] */
                           double* est_amp_sums_out,                 /* optional [n_points][4][N_carrier] */
                           double* err_sums_out,                     /* optional [n_points][4][N_carrier] */
                           double* amp_err_sums_out,                 /* optional [n_points][4][N_carrier] */
                           uint64_t* nmse_hist_out,                  /* optional [n_points][4][hist_bins] */
                           uint64_t* nmse_below_out,                 /* optional [n_points][4] */
                           uint64_t* nmse_above_out,                 /* optional [n_points][4] */
                           uint64_t* nmse_nan_out,                   /* optional [n_points][4] */
                           double* thresholds_out,                   /* optional HOST [hist_bins + 1] */
                           uint64_t* pick_hist_out,                  /* optional [n_points][K] */
                           double* tap_amp_sums_out,                 /* optional [n_points][K] */
                           uint64_t* n_picks_hist_out,               /* optional [n_points][T + 1] */
                           double* true_tap_amp_sums_out,            /* optional [n_points][K] */
                           uint64_t* true_outside_out,               /* optional [n_points] */
                           uint64_t* support_out,                    /* optional [n_points][3] */
                           int32_t* picks_out,                       /* optional [n_points][frames_per_point][T] */
                           void* tap_x_out,                          /* optional [n_points][frames_per_point][T] complex double */
                           int flags);

/* The fused generator with a given payload: ofdm_tx_frames_fused_ex (h, h_len) or ofdm_tx_frames_fading_ex (tap_delay, tap_power,
 * n_taps in place of h) with the payload draw replaced by the caller's bits -- what file_reader.m hands the chain of every driver
 * of the reference (T3/Main_model_Task_3.m:26-32).  payload: a packed bit stream where `flags` says, stream bit i in bit
 * 7 - i % 8 of byte i / 8 (the library's packing), ceil(n_bits / 8) bytes.  Frame f of the call carries the stream bits
 * (first_frame + f) frame_bits .. + frame_bits - 1 with frame_bits = nd N_symb bps, in general no multiple of 8; bits at or beyond
 * n_bits are 0 (the padding display_pic.m:5-6 assumes), a frame wholly beyond the payload is all zeros.  The noise, STO / CFO and
 * fading draws of frame f are those of Philox stream frame0 + f, as in the other generator entries: only the bit source changes.
 * For bits equal to the Philox payload of (seed, frame0 + f) every output equals the existing entry's, bit for bit.  With both
 * modes 0 and no sto_out / cfo_out the channel pass is that of ofdm_tx_frames_fused / _fading.  Outputs as there (taps_out only
 * with a tap-delay line).  OFDM_ERR_ARG, before anything is launched or written, in this order: payload given and n_bits >= 1;
 * first_frame 0 .. 2^32 - 1; h and taps together; what the generator entries refuse, in their order and words under the name
 * tx_frames_payload; a frame of more than 2^31 - 1 bits. */
int ofdm_tx_frames_payload(ofdm_rx_plan* plan, const uint8_t* payload, /* [ceil(n_bits / 8)], where flags says */
                           int64_t n_bits, int64_t first_frame,
                           const void* h, int h_len,                 /* HOST, complex in the plan's precision, or NULL / 0 */
                           const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                           double snr_db, uint64_t seed, int64_t frame0, int64_t n_frames,
                           const uint8_t* scr_reg15,                 /* HOST uint8[15] or NULL */
                           int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                           void* rx_out,                             /* [n_frames][frame_samples] */
                           uint8_t* ref_bits_out,                    /* optional [n_frames][frame_bytes] */
                           uint8_t* sc_ref_bits_out,                 /* optional [n_frames][frame_bytes], needs scr_reg15 */
                           double* taps_out,                         /* optional [n_frames][n_taps] complex double */
                           int64_t* sto_out, double* cfo_out,        /* optional [n_frames] */
                           int flags);

/* Payload transport as one device-resident call: the caller's bits through the generator and a receiver and back as one stream,
 * at every point of a sweep (T3/Main_model_Task_3.m:26-32, :160-185: file_reader.m -> the chain -> DeScrambler -> BER_func ->
 * display_pic.m).  Let F = ceil(n_bits / frame_bits).  For every point p and repeat r the frames i = 0 .. F - 1 of
 * ofdm_tx_frames_payload(payload, n_bits, first_frame = 0) with snr_db[p], seeds[p] on Philox stream frame0 + r F + i, decoded as
 * the matching sweep decodes them -- receiver 5: ofdm_rx_chain_task5 as in ofdm_ber_sweep_task5 / _fading (the plan's route, its
 * MMSE, h = ifft(H_LS) and OMP-route modes, the DeScrambler rule; sto_mode, cfo_mode, time_desync and freq_desync must be 0 and
 * mp_desync 1); receiver 4: ofdm_rx_chain_task4(time_desync, freq_desync, mp_desync) as in ofdm_ber_sweep_task4 / _fading.  No
 * sample and no bit leaves the device between the payload and the tables.
 *   decoded_out [n_points][repeats][ceil(n_bits / 8)]: the received stream, the frames' decisions joined at bit offset
 *     i frame_bits and cut at n_bits, packed as the payload; the spare bits of the last byte are 0.
 *   errors_out [n_points][repeats]: the wrong bits among the payload's n_bits, BER_func(input_bits, dsc_bits); the zero padding of
 *     the last frame is transmitted but not counted.  frame_errors_out [n_points][repeats][F]: per frame, over its share of n_bits.
 *   ones_out [n_points][n_bits]: the sum over the repeats of decoded bit i (the mean received picture is ones / repeats).
 * The outputs are overwritten.  Chunks of whole frames of one point's F repeats frames, which may cut a repeat, budgeted as the
 * matching sweep budgets them with the chunk's decisions beside them (max_frames_per_chunk > 0 caps the frames of a chunk); every
 * output is bitwise independent of the chunking.  With OFDM_DEVICE nothing synchronises the host, apart from a first-call growth
 * of the workspace.  OFDM_ERR_ARG, before anything is launched or written, in this order: receiver 4 / 5; plan and payload given;
 * the plan has data carriers; n_bits >= 1; repeats >= 1; F repeats and frame0 + F repeats inside the 32-bit stream range; h and
 * taps together; receiver 5 with an impairment or a flag ofdm_ber_sweep_task5 does not have; every refusal of the matching sweep
 * in its order and words under the name transport (the Task-4 sweep names itself ber_sweep_task4 behind its channel check); a
 * frame of more than 2^31 - 1 bits; an output is wanted. */
int ofdm_payload_transport(ofdm_rx_plan* plan, int receiver,      /* 4 | 5 */
                           const uint8_t* payload,                   /* [ceil(n_bits / 8)], where flags says */
                           int64_t n_bits, int64_t repeats,
                           const void* h, int h_len,                 /* HOST, complex in the plan's precision, or NULL / 0 */
                           const int32_t* tap_delay, const double* tap_power, int n_taps, /* HOST, or NULL / NULL / 0 */
                           int sto_mode, int64_t sto_value, int cfo_mode, double cfo_value,
                           int time_desync, int freq_desync, int mp_desync,
                           const double* snr_db, const uint64_t* seeds, /* HOST [n_points] */
                           int64_t n_points, int64_t frame0,
                           const uint8_t* scr_reg15,                 /* HOST uint8[15] or NULL */
                           int64_t max_frames_per_chunk,
                           uint8_t* decoded_out,                     /* optional [n_points][repeats][ceil(n_bits / 8)] */
                           uint64_t* errors_out,                     /* optional [n_points][repeats] */
                           uint32_t* frame_errors_out,               /* optional [n_points][repeats][F] */
                           uint32_t* ones_out,                       /* optional [n_points][n_bits] */
                           int flags);

#ifdef __cplusplus
}
#endif
#endif /* OFDM_MI355X_H */
