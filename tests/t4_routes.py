"""The route of the Task-4 receiver (csrc/t4_route.hpp: t4_route_choose) as a hand-written table.  TEST INFRASTRUCTURE: a helper
module (no tests here), imported by test_t4_route_host.py and test_gpu_task4_routes_parent.py.  Written from the dispatch rules
below, not by running the header.

A route in words:  acf form ifo demod est means channel pilots lazy x_stride eq
  acf      none (no sync flag) | search (t4_acf_search_kernel) | full (OFDM_T4_FULL_ACF: acf_kernel + acf_plateau_kernel + t4_scalars_kernel)
  form     direct (Nfft 512 .. 4096 without OFDM_T4_STAGED) | staged (t4_align_kernel first)
  ifo      none (no freq_desync) | wave (t4_ifo_wave_kernel) | segment_direct (t4_segment_direct_kernel, first_above_kernel,
           t4_ifo_finalize_kernel) | segment_staged (t4_segment_kernel, first_above_kernel, t4_ifo_kernel)
  demod    wave (fp32, Nfft 2048, even N_carrier <= 1024, no OFDM_T4_NO_WAVE) | demod<NW> (t4_demod_kernel, NW = Nfft / 512) |
           demod_device (staged)
  est      fused (t4_fine_est_kernel: direct form with a sync flag or mp_desync, no OFDM_T4_UNFUSED_SYNC) | tau_phase (fine_tau_kernel
           + fine_phase_kernel) | tau_phase_apply (+ fine_apply_kernel, staged) | none
  means    fused (in t4_fine_est_kernel) | kernel (t4_mean_pilots_kernel) | none (no mp_desync)
  channel  band (fp32 without OFDM_T4_DENSE_SPLINE) | dense (t4_apply_operator_kernel) | ones (no mp_desync)
  pilots   compact (the demodulator's [np x N_symb] rows, frame stride np * N_symb, direct) | grid (X, stride Nfft * N_symb, staged)
  lazy     1: fine_sync's rotation is applied where X is read (direct form with a sync flag), 0: not
  x_stride N_carrier (direct) | Nfft (staged): the equaliser's row count per symbol
  eq       vec (fp32, even N_carrier <= 2048, even x_stride) | scalar

The route factorises: STATIC holds the words a geometry and a precision fix, FLAGS the words the three flags (time_desync,
freq_desync, mp_desync) fix for either form.  "on" stands for the geometry's own word (its ifo kernel / band or dense)."""
import t4_cases as tc

# (case, precision) -> form, ifo when on, demod, channel when on, pilots, x_stride, eq
STATIC = {
    ("n64", "fp64"): ("staged", "segment_staged", "demod_device", "dense", "grid", 64, "scalar"),
    ("n64", "fp32"): ("staged", "segment_staged", "demod_device", "band", "grid", 64, "vec"),
    ("n64late", "fp64"): ("staged", "segment_staged", "demod_device", "dense", "grid", 64, "scalar"),
    ("n64late", "fp32"): ("staged", "segment_staged", "demod_device", "band", "grid", 64, "vec"),
    ("n256", "fp64"): ("staged", "segment_staged", "demod_device", "dense", "grid", 256, "scalar"),
    ("n256", "fp32"): ("staged", "segment_staged", "demod_device", "band", "grid", 256, "vec"),
    ("n512odd", "fp64"): ("direct", "segment_direct", "demod<1>", "dense", "compact", 201, "scalar"),
    ("n512odd", "fp32"): ("direct", "segment_direct", "demod<1>", "band", "compact", 201, "scalar"),      # odd N_carrier
    ("n1024tg100", "fp64"): ("direct", "segment_direct", "demod<2>", "dense", "compact", 400, "scalar"),
    ("n1024tg100", "fp32"): ("direct", "segment_direct", "demod<2>", "band", "compact", 400, "vec"),
    ("n2048odd", "fp64"): ("direct", "segment_direct", "demod<4>", "dense", "compact", 801, "scalar"),
    ("n2048odd", "fp32"): ("direct", "segment_direct", "demod<4>", "band", "compact", 801, "scalar"),     # odd: off the wave path
    ("n2048tg255", "fp64"): ("direct", "segment_direct", "demod<4>", "dense", "compact", 800, "scalar"),
    ("n2048tg255", "fp32"): ("direct", "wave", "wave", "band", "compact", 800, "vec"),
    ("n4096", "fp64"): ("direct", "segment_direct", "demod<8>", "dense", "compact", 1024, "scalar"),
    ("n4096", "fp32"): ("direct", "segment_direct", "demod<8>", "band", "compact", 1024, "vec"),
    ("n8192", "fp64"): ("staged", "segment_staged", "demod_device", "dense", "grid", 8192, "scalar"),
    ("n8192", "fp32"): ("staged", "segment_staged", "demod_device", "band", "grid", 8192, "vec"),
    # frames.config_C3(), the benchmark's Task-4 workload: Nfft 2048, T_guard 256, 800 carriers, 50 symbols
    ("C3", "fp64"): ("direct", "segment_direct", "demod<4>", "dense", "compact", 800, "scalar"),
    ("C3", "fp32"): ("direct", "wave", "wave", "band", "compact", 800, "vec"),
}

# form -> flags -> acf, ifo, est, means, channel, lazy
FLAGS = {
    "direct": {(1, 1, 1): ("search", "on", "fused", "fused", "on", 1),
               (1, 0, 1): ("search", "none", "fused", "fused", "on", 1),
               (0, 1, 0): ("search", "on", "fused", "none", "ones", 1),
               (0, 0, 1): ("none", "none", "fused", "fused", "on", 0),
               (0, 0, 0): ("none", "none", "none", "none", "ones", 0)},
    "staged": {(1, 1, 1): ("search", "on", "tau_phase_apply", "kernel", "on", 0),
               (1, 0, 1): ("search", "none", "tau_phase_apply", "kernel", "on", 0),
               (0, 1, 0): ("search", "on", "tau_phase_apply", "none", "ones", 0),
               (0, 0, 1): ("none", "none", "none", "kernel", "on", 0),
               (0, 0, 0): ("none", "none", "none", "none", "ones", 0)},
}


def expected_words(name, precision, flags):
    form, ifo_on, demod, channel_on, pilots, x_stride, eq = STATIC[name, precision]
    acf, ifo, est, means, channel, lazy = FLAGS[form][tuple(flags)]
    return " ".join(map(str, (acf, form, ifo_on if ifo == "on" else ifo, demod, est, means, channel_on if channel == "on" else channel,
                              pilots, lazy, x_stride, eq)))


# The switch-only runs, all with the flags (1, 1, 1): test_gpu_task4_sizes.SWITCH_RUNS and OFDM_T4_DENSE_SPLINE.
SWITCH_ROWS = [("OFDM_T4_UNFUSED_SYNC", "n1024tg100"), ("OFDM_T4_UNFUSED_SYNC", "n4096"), ("OFDM_T4_FULL_ACF", "n64"),
               ("OFDM_T4_FULL_ACF", "n8192"), ("OFDM_T4_STAGED", "n4096"), ("OFDM_T4_NO_WAVE", "n2048tg255"),
               ("OFDM_T4_DENSE_SPLINE", "n1024tg100")]
SWITCH_WORDS = {
    ("OFDM_T4_UNFUSED_SYNC", "n1024tg100", "fp64"): "search direct segment_direct demod<2> tau_phase kernel dense compact 1 400 scalar",
    ("OFDM_T4_UNFUSED_SYNC", "n1024tg100", "fp32"): "search direct segment_direct demod<2> tau_phase kernel band compact 1 400 vec",
    ("OFDM_T4_UNFUSED_SYNC", "n4096", "fp64"): "search direct segment_direct demod<8> tau_phase kernel dense compact 1 1024 scalar",
    ("OFDM_T4_UNFUSED_SYNC", "n4096", "fp32"): "search direct segment_direct demod<8> tau_phase kernel band compact 1 1024 vec",
    ("OFDM_T4_FULL_ACF", "n64", "fp64"): "full staged segment_staged demod_device tau_phase_apply kernel dense grid 0 64 scalar",
    ("OFDM_T4_FULL_ACF", "n64", "fp32"): "full staged segment_staged demod_device tau_phase_apply kernel band grid 0 64 vec",
    ("OFDM_T4_FULL_ACF", "n8192", "fp64"): "full staged segment_staged demod_device tau_phase_apply kernel dense grid 0 8192 scalar",
    ("OFDM_T4_FULL_ACF", "n8192", "fp32"): "full staged segment_staged demod_device tau_phase_apply kernel band grid 0 8192 vec",
    ("OFDM_T4_STAGED", "n4096", "fp64"): "search staged segment_staged demod_device tau_phase_apply kernel dense grid 0 4096 scalar",
    ("OFDM_T4_STAGED", "n4096", "fp32"): "search staged segment_staged demod_device tau_phase_apply kernel band grid 0 4096 vec",
    ("OFDM_T4_NO_WAVE", "n2048tg255", "fp64"): "search direct segment_direct demod<4> fused fused dense compact 1 800 scalar",
    ("OFDM_T4_NO_WAVE", "n2048tg255", "fp32"): "search direct segment_direct demod<4> fused fused band compact 1 800 vec",
    ("OFDM_T4_DENSE_SPLINE", "n1024tg100", "fp64"): "search direct segment_direct demod<2> fused fused dense compact 1 400 scalar",
    ("OFDM_T4_DENSE_SPLINE", "n1024tg100", "fp32"): "search direct segment_direct demod<2> fused fused dense compact 1 400 vec",
}

# The refusals, on the n64 geometry (Nfft 64, T_guard 8, 48 carriers, 12 symbols, 9 pilots) with one field changed:
# name -> (changed fields, flags, refusal id, message).  A frame of one symbol has no autocorrelation output (n_out = 0), so with
# freq_desync it meets the first refusal too: the second ("rx_signal(Nfft+1:2*Nfft) exceeds the frame", id ifo_segment) needs
# n_out > 0, i.e. two symbols, which hold 2 * Nfft samples -- no shape reaches it, in the parent either.
MSG_GUARD = "rx_chain_task4: frame shorter than T_guard + Nfft, or T_guard outside 1..1024"
MSG_IFO_SEGMENT = "rx_chain_task4: rx_signal(Nfft+1:2*Nfft) exceeds the frame"
MSG_PILOTS = "rx_chain_task4: fine_sync needs at least two pilot carriers"
REFUSALS = {
    "tg0": (dict(t_guard=0), (1, 1, 1), "guard", MSG_GUARD),
    "tg1025": (dict(t_guard=1025), (1, 1, 1), "guard", MSG_GUARD),
    "short_frame": (dict(n_symb=1), (1, 0, 1), "guard", MSG_GUARD),
    "one_symbol_freq_desync": (dict(n_symb=1), (0, 1, 1), "guard", MSG_GUARD),
    "one_pilot": (dict(np=1), (1, 1, 1), "pilots", MSG_PILOTS),
}


def flag_sets(name):
    return tc.flag_sets(tc.BY_NAME[name]) if name in tc.BY_NAME else tc.ALL_FLAGS
