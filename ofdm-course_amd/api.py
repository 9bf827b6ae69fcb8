"""Host-side mirror of the reference's operator interface (one Python function per `.m` file,
same names, argument order and error behaviour) on top of the C ABI of libofdm_mi355x.so.

Data arguments may be
  * numpy arrays  -> host-pointer flavour of the ABI (what a MEX gateway does): the library stages
    the data through HBM, runs the HIP kernels and copies the results back;
  * torch CUDA tensors -> device-pointer flavour: zero-copy, asynchronous on torch's current stream.

Precision follows the dtype of the primary argument: complex128/float64 -> fp64 kernels (parity
mode, MATLAB is double everywhere), complex64/float32 -> fp32 kernels (throughput mode).
Matrices use MATLAB shapes `[rows, cols]` and are handed to the library in column-major order.
Index vectors are the reference's 1-based carrier indices.

Nothing in this module computes on the CPU: every function ends in a C-ABI call, and a missing
library / GPU raises OfdmError.
"""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib as L
from ._lib import OfdmError  # noqa: F401

try:  # torch is optional plumbing (device memory + streams)
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = [
    "OfdmError", "init", "shutdown", "constellation_func", "mapping", "demapping", "Scrambler",
    "DeScrambler", "Scrambler_frames", "DeScrambler_frames", "OFDM_map_carriers", "get_payload",
    "OFDM_modulator", "OFDM_demodulator", "get_MP_channel_resp", "apply_channel", "Noise", "add_STO",
    "add_CFO", "add_STO_CFO_frames", "apply_channel_frames", "Noise_frames", "AutoCorrFunction", "remove_IFO", "fine_sync", "estimate_channel", "equalize_signal",
    "interpolate", "LS_CE", "MMSE_CE", "sensing_matrix", "MP_estimate", "OMP_estimate", "BER_func",
    "MER_func", "calculatePAPR", "calculate_window_PAPR", "calculateCCDF", "RxPlan", "rx_chain_task5", "rx_chain_task4", "rx_spectrum", "rx_acf", "rx_fine", "rx_ifo", "rx_hest", "bit_error_profile", "task5_part2_tile", "task5_mse_tile", "OMP_estimate_batch", "DEFAULT_REGISTER",
]

DEFAULT_REGISTER = (1, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0)   # T5/Main_model_Task_5.m:55


def init(device_id: int = -1):
    L.check(L.load().ofdm_init(int(device_id)), "ofdm_init")


def shutdown():
    L.check(L.load().ofdm_shutdown(), "ofdm_shutdown")


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


class _Call:
    """Marshals the arguments of one C-ABI call (placement + precision from the primary arg)."""

    def __init__(self, primary, f64=None):
        self.lib = L.load()
        self.dev = _is_torch(primary) and primary.is_cuda
        if _is_torch(primary) and not primary.is_cuda:
            primary = primary.numpy()
        if f64 is None:
            if _is_torch(primary):
                f64 = primary.dtype in (torch.complex128, torch.float64)
            else:
                dt = np.asarray(primary).dtype
                f64 = dt not in (np.complex64, np.float32)
        self.f64 = bool(f64)
        self.flags = (L.OFDM_F64 if self.f64 else L.OFDM_F32) | (L.OFDM_DEVICE if self.dev else L.OFDM_HOST)
        self.keep = []
        if self.dev:
            self.device = primary.device
            init(self.device.index if self.device.index is not None else torch.cuda.current_device())
            L.check(self.lib.ofdm_set_stream(C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                    "ofdm_set_stream")
        else:
            L.check(self.lib.ofdm_set_stream(None), "ofdm_set_stream")

    # ---- dtypes
    @property
    def cdt(self):
        return np.complex128 if self.f64 else np.complex64

    @property
    def tcdt(self):
        return torch.complex128 if self.f64 else torch.complex64

    # ---- inputs
    def _flat(self, x, npdt, tdt):
        if self.dev:
            if not _is_torch(x):
                x = torch.as_tensor(np.asarray(x))
            x = x.to(device=self.device, dtype=tdt)
            if x.ndim >= 2:
                x = x.movedim(tuple(range(x.ndim)), tuple(reversed(range(x.ndim)))).contiguous()
            else:
                x = x.contiguous()
            self.keep.append(x)
            return C.c_void_p(x.data_ptr()), x.numel()
        if _is_torch(x):
            x = x.cpu().numpy()
        a = np.ascontiguousarray(np.asarray(x, dtype=npdt).ravel(order="F"))
        self.keep.append(a)
        return a.ctypes.data_as(C.c_void_p), a.size

    def cin(self, x):
        return self._flat(x, self.cdt, self.tcdt if self.dev else None)[0]

    def bits_in(self, x):
        if self.dev and _is_torch(x):
            x = (x != 0)
        elif not self.dev:
            x = (np.asarray(x.cpu().numpy() if _is_torch(x) else x) != 0)
        return self._flat(x, np.uint8, torch.uint8 if self.dev else None)[0]

    def idx(self, v):
        """1-based index vector (MATLAB doubles) -> host int32 array."""
        if _is_torch(v):
            v = v.cpu().numpy()
        a = np.asarray(v).ravel()
        r = np.rint(a).astype(np.int32)
        if a.dtype.kind == "f" and not np.array_equal(r, a):
            raise OfdmError("index vector must hold integers")
        r = np.ascontiguousarray(r)
        self.keep.append(r)
        return r.ctypes.data_as(C.c_void_p), r.size

    # ---- outputs
    def cout(self, shape):
        return self._out(shape, self.cdt, self.tcdt if self.dev else None)

    def bits_out(self, n):
        return self._out((int(n),), np.uint8, torch.uint8 if self.dev else None)

    def _out(self, shape, npdt, tdt):
        shape = tuple(int(s) for s in shape)
        if self.dev:
            t = torch.empty(tuple(reversed(shape)), dtype=tdt, device=self.device)
            view = t.movedim(tuple(range(t.ndim)), tuple(reversed(range(t.ndim)))) if t.ndim >= 2 else t
            self.keep.append(t)
            return view, C.c_void_p(t.data_ptr())
        a = np.empty(shape, dtype=npdt, order="F")
        return a, a.ctypes.data_as(C.c_void_p)


def _shape2(x):
    s = tuple(x.shape)
    if len(s) == 1:
        return (s[0], 1)
    if len(s) != 2:
        raise OfdmError("expected a vector or a matrix")
    return s


def _cstr(s):
    return str(s).encode()


# ------------------------------------------------------------------------------------------------
# constellation / mapping / demapping
# ------------------------------------------------------------------------------------------------

def constellation_func(Constellation):
    """T5/constellation_func.m:4-35 -> (Dictionary[2^bps] complex128, Bit_depth_Dict)."""
    lib = L.load()
    d = np.empty(256, dtype=np.complex128)
    bps = C.c_int(0)
    L.check(lib.ofdm_constellation_func(_cstr(Constellation), d.ctypes.data_as(C.c_void_p), C.byref(bps), L.OFDM_F64),
            "constellation_func")
    return d[: 1 << bps.value].copy(), bps.value


def _bps(constellation):
    bps = C.c_int(0)
    L.check(L.load().ofdm_constellation_func(_cstr(constellation), None, C.byref(bps), 0), "constellation_func")
    return bps.value


def mapping(bits, constellation, precision="fp64"):
    """T5/mapping.m:1-25 -> (IQ row, pad).  Row input that needs padding is an error (mapping.m:11)."""
    bps = _bps(constellation)
    shp = tuple(bits.shape)
    n = int(np.prod(shp)) if len(shp) else 1
    is_row = len(shp) == 2 and shp[0] == 1 and shp[1] > 1
    if n % bps != 0 and is_row:
        raise OfdmError("mapping: vertcat dimension mismatch (row input needs padding)")
    call = _Call(bits if _is_torch(bits) else np.zeros(1, np.complex128 if precision == "fp64" else np.complex64),
                 f64=(precision == "fp64"))
    pb = call.bits_in(bits)
    n_iq = (n + bps - 1) // bps
    iq, piq = call.cout((n_iq,))
    pad = C.c_int(0)
    L.check(call.lib.ofdm_mapping(pb, n, _cstr(constellation), piq, C.byref(pad), call.flags), "mapping")
    return iq, pad.value


def demapping(pad, IQ, Constellation):
    """T5/demapping.m:1-25 -> bit row (uint8 0/1)."""
    bps = _bps(Constellation)
    call = _Call(IQ)
    n = int(np.prod(tuple(IQ.shape)))
    nb = n * bps - (int(pad) if pad != -1 else 0)
    if nb < 0:
        raise OfdmError("demapping: pad larger than the bit count")
    out, pout = call.bits_out(nb)
    L.check(call.lib.ofdm_demapping(int(pad), call.cin(IQ), n, _cstr(Constellation), pout, call.flags), "demapping")
    return out


# ------------------------------------------------------------------------------------------------
# scrambler
# ------------------------------------------------------------------------------------------------

def _scr(fn_name, Register, sequence):
    call = _Call(sequence if _is_torch(sequence) else np.zeros(1, np.complex64), f64=False)
    reg = np.ascontiguousarray((np.asarray(Register).ravel() != 0).astype(np.uint8))
    if reg.size != 15:
        raise OfdmError(f"{fn_name}: Register must have 15 elements")
    n = int(np.prod(tuple(sequence.shape)))
    out, pout = call.bits_out(n)
    fn = getattr(call.lib, "ofdm_" + fn_name)
    L.check(fn(reg.ctypes.data_as(C.c_void_p), call.bits_in(sequence), n, pout, call.flags), fn_name)
    return out, reg


def Scrambler(Register, sequence):
    """T5/Scrambler.m:1-28 -> (sc_sequence, Register)."""
    return _scr("Scrambler", Register, sequence)


def DeScrambler(Register, sequence):
    """T5/DeScrambler.m:1-28 -> (dsc_sequence, Register)."""
    return _scr("DeScrambler", Register, sequence)


def _scr_frames(fn_name, Register, seq_matrix):
    call = _Call(seq_matrix if _is_torch(seq_matrix) else np.zeros(1, np.complex64), f64=False)
    reg = np.ascontiguousarray((np.asarray(Register).ravel() != 0).astype(np.uint8))
    flen, nfr = _shape2(seq_matrix)
    out, pout = call._out((flen, nfr), np.uint8, torch.uint8 if call.dev else None)
    fn = getattr(call.lib, "ofdm_" + fn_name)
    L.check(fn(reg.ctypes.data_as(C.c_void_p), call.bits_in(seq_matrix), flen, nfr, pout, call.flags), fn_name)
    return out


def Scrambler_frames(Register, seq_matrix):
    """Per-frame loop of T5/Main_model_Task_5.m:58-69: one column per frame, register reset per column."""
    return _scr_frames("Scrambler_frames", Register, seq_matrix)


def DeScrambler_frames(Register, seq_matrix):
    """Per-frame loop of T5/Main_model_Task_5.m:260-271."""
    return _scr_frames("DeScrambler_frames", Register, seq_matrix)


# ------------------------------------------------------------------------------------------------
# carriers, modulator, demodulator
# ------------------------------------------------------------------------------------------------

def OFDM_map_carriers(QAM_payload, N_symb, Nfft, dataCarriers, pilotCarriers, pilotValues):
    """T5/OFDM_map_carriers.m:2-9."""
    call = _Call(QAM_payload)
    N_symb, Nfft = int(N_symb), int(Nfft)
    pdc, nd = call.idx(dataCarriers)
    ppc, npil = call.idx(pilotCarriers)
    n_pay = int(np.prod(tuple(QAM_payload.shape)))
    if n_pay != nd * N_symb:
        raise OfdmError("OFDM_map_carriers: reshape size mismatch (payload != numel(dataCarriers)*N_symb)")
    pv_n = int(np.prod(tuple(pilotValues.shape))) if hasattr(pilotValues, "shape") else 1
    scalar = 1 if pv_n == 1 else 0
    if not scalar and pv_n != npil * N_symb:
        raise OfdmError("OFDM_map_carriers: pilotValues must be [numel(pilotCarriers) x N_symb] or scalar")
    pv = pilotValues if hasattr(pilotValues, "shape") else np.asarray([pilotValues])
    out, pout = call.cout((Nfft, N_symb))
    L.check(call.lib.ofdm_OFDM_map_carriers(call.cin(QAM_payload), N_symb, Nfft, pdc, nd, ppc, npil,
                                            call.cin(pv), scalar, pout, call.flags), "OFDM_map_carriers")
    return out


def get_payload(RX_OFDM_symbols, dataCarriers):
    """T5/get_payload.m:2-4."""
    call = _Call(RX_OFDM_symbols)
    nfft, ns = _shape2(RX_OFDM_symbols)
    pdc, nd = call.idx(dataCarriers)
    out, pout = call.cout((nd, ns))
    L.check(call.lib.ofdm_get_payload(call.cin(RX_OFDM_symbols), nfft, ns, pdc, nd, pout, call.flags), "get_payload")
    return out


def OFDM_modulator(OFDM_symbols, T_guard):
    """T5/OFDM_modulator.m:2-11."""
    call = _Call(OFDM_symbols)
    nfft, ns = _shape2(OFDM_symbols)
    tg = int(T_guard)
    out, pout = call.cout((nfft + tg, ns))
    L.check(call.lib.ofdm_OFDM_modulator(call.cin(OFDM_symbols), pout, nfft, ns, tg, call.flags), "OFDM_modulator")
    return out


def OFDM_demodulator(OFDM_time_guarded, T_guard):
    """T5/OFDM_demodulator.m:2-10."""
    call = _Call(OFDM_time_guarded)
    rows, ns = _shape2(OFDM_time_guarded)
    tg = int(T_guard)
    nfft = rows - tg
    out, pout = call.cout((nfft, ns))
    L.check(call.lib.ofdm_OFDM_demodulator(call.cin(OFDM_time_guarded), pout, nfft, ns, tg, call.flags),
            "OFDM_demodulator")
    return out


# ------------------------------------------------------------------------------------------------
# channel side
# ------------------------------------------------------------------------------------------------

def get_MP_channel_resp(channel_taps, Nfft):
    """T5/get_MP_channel_resp.m:2-19 -> (impulse_response row, frequency_response row), complex128."""
    lib = L.load()
    init()
    taps = np.atleast_2d(np.asarray(channel_taps))
    nt = taps.shape[0]
    t_re = np.ascontiguousarray(np.real(taps).astype(np.float64).ravel(order="F"))
    t_im = np.ascontiguousarray(np.imag(taps[:, 1]).astype(np.float64)) if np.iscomplexobj(taps) else None
    maxd = int(np.max(np.real(taps[:, 0])))
    h = np.empty(maxd + 1, dtype=np.complex128)
    H = np.empty(int(Nfft), dtype=np.complex128)
    hl = C.c_int(0)
    L.check(lib.ofdm_get_MP_channel_resp(t_re.ctypes.data_as(C.c_void_p),
                                         t_im.ctypes.data_as(C.c_void_p) if t_im is not None else None,
                                         nt, int(Nfft), h.ctypes.data_as(C.c_void_p), C.byref(hl),
                                         H.ctypes.data_as(C.c_void_p), L.OFDM_F64), "get_MP_channel_resp")
    return h[: hl.value], H


def apply_channel(x, h):
    """conv(x, h.', 'full')(1:numel(x)) -- T5/Main_model_Task_5.m:126-127."""
    call = _Call(x)
    n = int(np.prod(tuple(x.shape)))
    hh = np.ascontiguousarray(np.asarray(h.cpu().numpy() if _is_torch(h) else h).ravel().astype(call.cdt))
    out, pout = call.cout((n,))
    L.check(call.lib.ofdm_channel_conv(call.cin(x), n, hh.ctypes.data_as(C.c_void_p), hh.size, pout, call.flags),
            "channel_conv")
    return out


def Noise(SNR, IQ_TX, seed=0, stream=0):
    """T5/Noise.m:1-12 with the build's counter-based generator -> (IQ_RX, N_var)."""
    call = _Call(IQ_TX)
    n = int(np.prod(tuple(IQ_TX.shape)))
    out, pout = call.cout(tuple(IQ_TX.shape) if len(IQ_TX.shape) <= 2 else (n,))
    nv = C.c_double(0)
    L.check(call.lib.ofdm_Noise(float(SNR), call.cin(IQ_TX), n, int(seed), int(stream), pout, C.byref(nv), call.flags),
            "Noise")
    return out, nv.value


def apply_channel_frames(x, h):
    """apply_channel on every column of x = [frame_len, n_frames] independently (Monte-Carlo frames)."""
    call = _Call(x)
    flen, nfr = _shape2(x)
    hh = np.ascontiguousarray(np.asarray(h.cpu().numpy() if _is_torch(h) else h).ravel().astype(call.cdt))
    out, pout = call.cout((flen, nfr))
    L.check(call.lib.ofdm_channel_conv_frames(call.cin(x), flen, nfr, hh.ctypes.data_as(C.c_void_p), hh.size, pout,
                                              call.flags), "channel_conv_frames")
    return out


def Noise_frames(SNR, IQ_TX, seed=0, stream0=0):
    """Noise() applied per column of IQ_TX = [frame_len, n_frames]; column f uses Philox stream stream0+f."""
    call = _Call(IQ_TX)
    flen, nfr = _shape2(IQ_TX)
    out, pout = call.cout((flen, nfr))
    L.check(call.lib.ofdm_Noise_frames(float(SNR), call.cin(IQ_TX), flen, nfr, int(seed), int(stream0), pout,
                                       call.flags), "Noise_frames")
    return out


def add_STO(y, nSTO):
    """T5/add_STO.m:1-10."""
    call = _Call(y)
    n = int(np.prod(tuple(y.shape)))
    out, pout = call.cout((n,))
    L.check(call.lib.ofdm_add_STO(call.cin(y), n, int(nSTO), pout, call.flags), "add_STO")
    return out


def add_STO_CFO_frames(y, nSTO=None, CFO=None, Nfft=1):
    """add_STO then add_CFO per frame of y [frame_len, n_frames] (column = frame), every frame with its own nSTO[f] / CFO[f]
    (T4/Main_model_Task_4.m:101-110 per Monte-Carlo run); None leaves a stage out."""
    call = _Call(y)
    frame_len, n_frames = _shape2(y)
    out, pout = call.cout((frame_len, n_frames))
    ps = pc = None
    if nSTO is not None:
        ps = call._flat(nSTO, np.int64, torch.int64 if call.dev else None)[0]
    if CFO is not None:
        pc = call._flat(CFO, np.float64, torch.float64 if call.dev else None)[0]
    L.check(call.lib.ofdm_add_STO_CFO_frames(call.cin(y), frame_len, n_frames, ps, pc, int(Nfft), pout, call.flags),
            "add_STO_CFO_frames")
    return out


def add_CFO(y, CFO, Nfft):
    """T5/add_CFO.m:1-8."""
    call = _Call(y)
    n = int(np.prod(tuple(y.shape)))
    out, pout = call.cout((n,))
    L.check(call.lib.ofdm_add_CFO(call.cin(y), n, float(CFO), int(Nfft), pout, call.flags), "add_CFO")
    return out


# ------------------------------------------------------------------------------------------------
# synchronisation
# ------------------------------------------------------------------------------------------------

def AutoCorrFunction(RxSignal, WidthWindow, Nfft):
    """T5/AutoCorrFunction.m:1-28 -> (AutoCorr row, TgPosition, FreqOffset).

    Issues the reference's warning and returns TgPosition = 65 when no plateau is found."""
    call = _Call(RxSignal)
    n = int(np.prod(tuple(RxSignal.shape)))
    W, Nfft = int(WidthWindow), int(Nfft)
    n_out = max(n - W - Nfft, 0)
    rho, prho = call.cout((n_out,))
    pos = C.c_int64(0)
    fo = C.c_double(0)
    rc = L.check(call.lib.ofdm_AutoCorrFunction(call.cin(RxSignal), n, W, Nfft, prho, C.byref(pos), C.byref(fo),
                                                call.flags), "AutoCorrFunction")
    if rc == L.OFDM_SOFT_ACF_FALLBACK:
        warnings.warn("AutoCorrFunction: problem locating the guard interval; TgPosition = 65")
    return rho, int(pos.value), fo.value


def remove_IFO(rx_signal, Nfft):
    """T5/remove_IFO.m:1-11 -> (fixed_rx_signal, IFO)."""
    call = _Call(rx_signal)
    n = int(np.prod(tuple(rx_signal.shape)))
    out, pout = call.cout((n,))
    ifo = C.c_int(0)
    L.check(call.lib.ofdm_remove_IFO(call.cin(rx_signal), n, int(Nfft), pout, C.byref(ifo), call.flags), "remove_IFO")
    return out, ifo.value


def fine_sync(rx_signal, pilotCarriers, pilotValues, time_desync, freq_desync, variant="T5", return_estimates=False):
    """T5/fine_sync.m:1-45 (variant='T4' -> T4/fine_sync.m)."""
    call = _Call(rx_signal)
    nfft, ns = _shape2(rx_signal)
    ppc, npil = call.idx(pilotCarriers)
    out, pout = call.cout((nfft, ns))
    tau, ph = C.c_double(0), C.c_double(0)
    L.check(call.lib.ofdm_fine_sync(call.cin(rx_signal), nfft, ns, ppc, npil, call.cin(pilotValues),
                                    int(bool(time_desync)), int(bool(freq_desync)), 1 if variant == "T4" else 0,
                                    pout, C.byref(tau), C.byref(ph), call.flags), "fine_sync")
    if return_estimates:
        return out, tau.value, ph.value
    return out


# ------------------------------------------------------------------------------------------------
# channel estimation / equalisation
# ------------------------------------------------------------------------------------------------

def interpolate(H, pilot_loc, Nfft, method):
    """T5/interpolate.m:1-24."""
    call = _Call(H)
    ploc, npil = call.idx(pilot_loc)
    out, pout = call.cout((int(Nfft),))
    L.check(call.lib.ofdm_interpolate(call.cin(H), ploc, npil, int(Nfft), str(method)[0].lower().encode(), pout,
                                      call.flags), "interpolate")
    return out


def estimate_channel(rx_signal, allCarriers, pilotCarriers, pilotValues):
    """T5/estimate_channel.m:1-9 -> (H_est row over allCarriers, Hest_at_pilots column)."""
    call = _Call(rx_signal)
    nfft, ns = _shape2(rx_signal)
    pall, nall = call.idx(allCarriers)
    ppc, npil = call.idx(pilotCarriers)
    h, ph = call.cout((nall,))
    hp, php = call.cout((npil,))
    L.check(call.lib.ofdm_estimate_channel(call.cin(rx_signal), nfft, ns, pall, nall, ppc, npil,
                                           call.cin(pilotValues), ph, php, call.flags), "estimate_channel")
    return h, hp


def equalize_signal(OFDM_demod, Hest, N_carrier):
    """T5/equalize_signal.m:1-8."""
    call = _Call(OFDM_demod)
    nfft, ns = _shape2(OFDM_demod)
    nc = int(N_carrier)
    nh = int(np.prod(tuple(Hest.shape)))
    if nh < nc:
        raise OfdmError("equalize_signal: index exceeds the number of elements of Hest")
    hflat = Hest.reshape(-1)[:nc] if _is_torch(Hest) else np.asarray(Hest).ravel()[:nc]
    out, pout = call.cout((nfft, ns))
    L.check(call.lib.ofdm_equalize_signal(call.cin(OFDM_demod), nfft, ns, call.cin(hflat), nc, pout, call.flags),
            "equalize_signal")
    return out


def LS_CE(Y, Xp, pilot_loc, N_carrier):
    """T5/LS_CE.m:1-34."""
    call = _Call(Y)
    nfft, ns = _shape2(Y)
    ploc, npil = call.idx(pilot_loc)
    out, pout = call.cout((int(N_carrier),))
    L.check(call.lib.ofdm_LS_CE(call.cin(Y), nfft, ns, call.cin(Xp), ploc, npil, int(N_carrier), pout, call.flags),
            "LS_CE")
    return out


def MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR):
    """T5/MMSE_CE.m:1-39."""
    call = _Call(Y)
    nfft, ns = _shape2(Y)
    ploc, npil = call.idx(pilot_loc)
    nh = int(np.prod(tuple(h.shape)))
    out, pout = call.cout((int(N_carrier),))
    L.check(call.lib.ofdm_MMSE_CE(call.cin(Y), nfft, ns, call.cin(Xp), ploc, npil, int(N_carrier), call.cin(h), nh,
                                  float(SNR), pout, call.flags), "MMSE_CE")
    return out


def sensing_matrix(pilotCarriers, Nfft, K, precision="fp64", device=None):
    """S = P*F(:,1:K) of T5/Main_model_Task_5.m:182-190 in closed form (never builds dftmtx)."""
    prim = (torch.zeros(1, dtype=torch.complex128 if precision == "fp64" else torch.complex64, device=device)
            if device is not None else np.zeros(1, np.complex128 if precision == "fp64" else np.complex64))
    call = _Call(prim)
    ppc, npil = call.idx(pilotCarriers)
    out, pout = call.cout((npil, int(K)))
    L.check(call.lib.ofdm_sensing_matrix(ppc, npil, int(Nfft), int(K), pout, call.flags), "sensing_matrix")
    return out


def MP_estimate(Y, sensing_matrix_, Nfft, dominant_taps, return_picks=False):
    """T5/MP_estimate.m:1-34 -> (H_MP row, h_impulse_est column)."""
    call = _Call(Y)
    npil, k = _shape2(sensing_matrix_)
    T = int(dominant_taps)
    H, pH = call.cout((int(Nfft),))
    h, ph = call.cout((int(Nfft),))
    picks = np.zeros(max(T, 1), dtype=np.int32)
    L.check(call.lib.ofdm_MP_estimate(call.cin(Y), call.cin(sensing_matrix_), npil, k, int(Nfft), T, pH, ph,
                                      picks.ctypes.data_as(C.c_void_p), call.flags), "MP_estimate")
    if return_picks:
        return H, h, picks[:T]
    return H, h


def OMP_estimate(Y, sensing_matrix_, Nfft, dominant_taps, SNR_dB=0.0):
    """T5/OMP_estimate.m:1-37 -> (H_OMP row, h_impulse_est row, index)."""
    call = _Call(Y)
    npil, k = _shape2(sensing_matrix_)
    T = int(dominant_taps)
    H, pH = call.cout((int(Nfft),))
    h, ph = call.cout((int(Nfft),))
    index = np.zeros(max(T, 1), dtype=np.int32)
    n_idx = C.c_int(0)
    L.check(call.lib.ofdm_OMP_estimate(call.cin(Y), call.cin(sensing_matrix_), npil, k, int(Nfft), T, float(SNR_dB),
                                       pH, ph, index.ctypes.data_as(C.c_void_p), C.byref(n_idx), call.flags),
            "OMP_estimate")
    return H, h, index[: n_idx.value].astype(np.int64)


# ------------------------------------------------------------------------------------------------
# metrics
# ------------------------------------------------------------------------------------------------

def BER_func(Bit_Tx, Bit_Rx, return_count=False):
    """T5/BER_func.m:1-7."""
    call = _Call(Bit_Tx if _is_torch(Bit_Tx) else np.zeros(1, np.complex64), f64=False)
    n = int(np.prod(tuple(Bit_Tx.shape)))
    if int(np.prod(tuple(Bit_Rx.shape))) != n:
        raise OfdmError("BER_func: arrays have incompatible sizes")
    ne = C.c_int64(0)
    L.check(call.lib.ofdm_BER_func(call.bits_in(Bit_Tx), call.bits_in(Bit_Rx), n, C.byref(ne), call.flags), "BER_func")
    if return_count:
        return ne.value
    return ne.value / n


def MER_func(IQ_RX, Constellation):
    """T5/MER_func.m:1-26."""
    call = _Call(IQ_RX)
    n = int(np.prod(tuple(IQ_RX.shape)))
    mer = C.c_double(0)
    L.check(call.lib.ofdm_MER_func(call.cin(IQ_RX), n, _cstr(Constellation), C.byref(mer), call.flags), "MER_func")
    return mer.value


# ------------------------------------------------------------------------------------------------
# PAPR study (Task 2)
# ------------------------------------------------------------------------------------------------

def calculatePAPR(OFDM_signal):
    """T2/calculatePAPR.m:2-11 -> PAPR in dB (host scalar)."""
    call = _Call(OFDM_signal)
    n = int(np.prod(tuple(OFDM_signal.shape)))
    v = C.c_double(0)
    L.check(call.lib.ofdm_calculatePAPR(call.cin(OFDM_signal), n, C.byref(v), call.flags), "calculatePAPR")
    return v.value


def calculate_window_PAPR(Tx_OFDM_Signal, Nfft):
    """T2/calculate_window_PAPR.m:2-15 -> PAPRs row (float64, length(signal) - Nfft + 1 entries)."""
    call = _Call(Tx_OFDM_Signal)
    n = int(np.prod(tuple(Tx_OFDM_Signal.shape)))
    n_out = max(n - int(Nfft) + 1, 0)
    out, pout = call._out((n_out,), np.float64, torch.float64 if call.dev else None)
    L.check(call.lib.ofdm_calculate_window_PAPR(call.cin(Tx_OFDM_Signal), n, int(Nfft), pout, call.flags),
            "calculate_window_PAPR")
    return out


def calculateCCDF(PAPR_values):
    """T2/calculateCCDF.m:2-6 -> (PAPR_ccdf, CCDF): ecdf abscissae (smallest value twice) and 1 - F."""
    call = _Call(PAPR_values, f64=True)
    n = int(np.prod(tuple(PAPR_values.shape)))
    pv = call._flat(PAPR_values, np.float64, torch.float64 if call.dev else None)[0]
    x, px = call._out((n + 1,), np.float64, torch.float64 if call.dev else None)
    c, pc = call._out((n + 1,), np.float64, torch.float64 if call.dev else None)
    n_out = C.c_int64(0)
    L.check(call.lib.ofdm_calculateCCDF(pv, n, px, pc, C.byref(n_out), call.flags), "calculateCCDF")
    return x[: n_out.value], c[: n_out.value]


# ------------------------------------------------------------------------------------------------
# fused Task-5 RX chain
# ------------------------------------------------------------------------------------------------

def _imp_mode(v, what):
    """Time_Delay / Freq_Shift argument -> (mode, value): None = off (0), a number = fixed (1), "random" = drawn (2)."""
    if v is None:
        return 0, 0
    if isinstance(v, str):
        if v != "random":
            raise OfdmError(f"{what}: Time_Delay / Freq_Shift must be None, a number or 'random'")
        return 2, 0
    return 1, v


def _torch_dtype(npdt):
    """The torch dtype of a device output declared with numpy dtype `npdt`: a wide unsigned type becomes the signed type of
    its width (uint64 counters -> int64, uint32 -> int32)."""
    dt = np.dtype(npdt)
    if dt.kind == "u" and dt.itemsize > 1:
        dt = np.dtype(f"i{dt.itemsize}")
    return torch.from_numpy(np.empty(0, dt)).dtype


class RxPlan:
    """Device-resident description of one Task-5 RX configuration (ofdm_rx_plan_create)."""

    def __init__(self, Nfft, T_guard, N_symb, N_carrier, pilotCarriers, dataCarriers, pilotValues_col, K,
                 dominant_taps, Constellation, precision="fp32", device=None):
        self.lib = L.load()
        init(-1 if device is None else int(device))
        self.f64 = precision == "fp64"
        self.Nfft, self.T_guard, self.N_symb, self.N_carrier = int(Nfft), int(T_guard), int(N_symb), int(N_carrier)
        self.K, self.taps = int(K), int(dominant_taps)
        self.bps = _bps(Constellation)
        pc = np.ascontiguousarray(np.rint(np.asarray(pilotCarriers).ravel()).astype(np.int32))
        dc = np.ascontiguousarray(np.rint(np.asarray(dataCarriers).ravel()).astype(np.int32))
        pv = np.ascontiguousarray(np.asarray(pilotValues_col).ravel().astype(np.complex128 if self.f64 else np.complex64))
        if pv.size != pc.size:
            raise OfdmError("RxPlan: pilotValues_col must have numel(pilotCarriers) entries")
        self.n_pilots, self.n_data = pc.size, dc.size
        self.dataCarriers = dc.copy()                              # 1-based, the order of the packed bits (error_study)
        h = C.c_void_p(None)
        L.check(self.lib.ofdm_rx_plan_create(C.byref(h), self.Nfft, self.T_guard, self.N_symb, self.N_carrier,
                                             pc.ctypes.data_as(C.c_void_p), pc.size, dc.ctypes.data_as(C.c_void_p),
                                             dc.size, pv.ctypes.data_as(C.c_void_p), self.K, self.taps,
                                             _cstr(Constellation), L.OFDM_F64 if self.f64 else L.OFDM_F32),
                "rx_plan_create")
        self.handle = h
        self.frame_bytes = int(self.lib.ofdm_rx_plan_frame_bytes(h))
        self.frame_bits = self.n_data * self.N_symb * self.bps
        self.frame_samples = (self.Nfft + self.T_guard) * self.N_symb

    def set_mmse(self, h=None, SNR=0.0):
        """Switch the plan's estimator to MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR) (T5/MMSE_CE.m:1-39) for
        every frame of a batch; `h=None` returns to OMP_estimate.  h: the impulse response handed to MMSE_CE."""
        if h is None:
            L.check(self.lib.ofdm_rx_plan_set_mmse(self.handle, None, 0, 0.0, L.OFDM_F64), "rx_plan_set_mmse")
            return
        hh = np.ascontiguousarray(np.asarray(h.cpu().numpy() if _is_torch(h) else h).ravel().astype(np.complex128))
        L.check(self.lib.ofdm_rx_plan_set_mmse(self.handle, hh.ctypes.data_as(C.c_void_p), hh.size, float(SNR),
                                               L.OFDM_F64 | L.OFDM_HOST), "rx_plan_set_mmse")

    def set_mmse_ls(self, SNR=None):
        """Switch the plan's estimator to the MMSE_CE call of T5/Main_model_Task_5.m:178-180 (ofdm_rx_plan_set_mmse_ls): per
        frame H_LS = LS_CE(...), h = ifft(H_LS), H = MMSE_CE(Y, Xp, pilot_loc, Nfft, N_carrier, h, SNR) -- no channel is
        supplied.  rx_chain_task5 uses `SNR`; ber_sweep uses each point's own SNR.  `SNR=None` returns to OMP_estimate.
        set_mmse and set_mmse_ls exclude each other: setting one clears the other."""
        L.check(self.lib.ofdm_rx_plan_set_mmse_ls(self.handle, 0 if SNR is None else 1, 0.0 if SNR is None else float(SNR)),
                "rx_plan_set_mmse_ls")

    def set_omp_route(self, route):
        """The OMP stage of rx_chain_task5 and ber_sweep on this plan (ofdm_rx_plan_set_omp_route), in the words of
        OMP_estimate_batch(route=): "batch" (a new plan: omp_batch_kernel or the fused symbol-1 + OMP launch, as ever), "auto"
        (the same wherever omp_batch_kernel's state fits the LDS, else omp_wide_kernel: K = Nfft on a random pilot mask,
        T5/Task5_part2.m:58-64,:181-184) or "wide" (always rx_pilot_kernel -> omp_wide_kernel -> the symbol stage).  A shape
        the chosen kernel cannot serve makes the receiver call raise OfdmError; the MMSE modes ignore the route."""
        if route not in _OMP_ROUTES:
            raise OfdmError(f"set_omp_route: route must be one of {sorted(_OMP_ROUTES)}")
        L.check(self.lib.ofdm_rx_plan_set_omp_route(self.handle, _OMP_ROUTES[route]), "rx_plan_set_omp_route")

    def _omp_route_get(self):
        r, last = C.c_int(0), C.c_int(0)
        L.check(self.lib.ofdm_rx_plan_get_omp_route(self.handle, C.byref(r), C.byref(last)), "rx_plan_get_omp_route")
        return r.value, last.value

    @property
    def omp_route(self):
        """The route set_omp_route left the plan in: "auto", "batch" or "wide"."""
        return _OMP_ROUTE_NAMES[self._omp_route_get()[0]]

    @property
    def last_omp_route(self):
        """The kernel the OMP stage of the last rx_chain_task5 / ber_sweep call ran: "batch" (the fused launch included), "wide",
        or None (MMSE mode, the generic entry, no call yet)."""
        return {1: "batch", 2: "wide"}.get(self._omp_route_get()[1])

    def set_descrambler(self, Register=None):
        """Per-frame DeScrambler(Register, .) inside rx_chain_task5 / rx_chain_task4 (T5/Main_model_Task_5.m:257-274): the
        demapped bits of every frame are descrambled in the pack stage before they are written / compared.  None = off."""
        if Register is None:
            L.check(self.lib.ofdm_rx_plan_set_descrambler(self.handle, None), "rx_plan_set_descrambler")
            return
        reg = np.ascontiguousarray(np.asarray(Register).ravel().astype(np.uint8))
        if reg.size != 15:
            raise OfdmError("set_descrambler: Register must have 15 entries")
        L.check(self.lib.ofdm_rx_plan_set_descrambler(self.handle, reg.ctypes.data_as(C.c_void_p)), "rx_plan_set_descrambler")

    def tx_frames(self, n_frames, h=None, SNR=None, seed=1, frame0=0, device=None, want_bits=False, Register=None,
                  Time_Delay=None, Freq_Shift=None, noise_first=False, want_draws=False):
        """Synthetic RX frames of this plan's geometry generated on the device (ofdm_tx_frames_ex): payload ->
        [Scrambler(Register, .) per frame] -> mapping -> OFDM_map_carriers -> OFDM_modulator -> channel stages.
        noise_first=True is the reference's order (T5/Main_model_Task_5.m:106-127, T4/Main_model_Task_4.m:94-110,:257-267):
        Noise(SNR) -> add_STO -> add_CFO -> conv(h); the default (False) is add_STO -> add_CFO -> conv(h) -> Noise(SNR).
        h=None: no channel; SNR=None: no noise.  Time_Delay / Freq_Shift: None = off, a number = that value for every
        frame, "random" = the per-frame draw of T4/Main_model_Task_4.m:101-110.
        Returns dict(rx=[frame_samples, n_frames], packed=[n_frames, frame_bytes] (the payload bits)
        (+ bits=[n_frames, frame_bits]) (+ sc_packed = the scrambled bits when Register is given)
        (+ Time_Delay [n_frames] int64, Freq_Shift [n_frames] float64 with want_draws));
        torch CUDA tensors when `device` is given, numpy arrays otherwise."""
        n_frames = int(n_frames)
        scr = Register is not None
        (rx, packed, bits, scp, sto, cfo), ptrs, flags = self._outputs(
            device, ((n_frames, self.frame_samples), np.complex128 if self.f64 else np.complex64),
            ((n_frames, self.frame_bytes), np.uint8), ((n_frames, self.frame_bits), np.uint8) if want_bits else None,
            ((n_frames, self.frame_bytes), np.uint8) if scr else None, ((n_frames,), np.int64) if want_draws else None,
            ((n_frames,), np.float64) if want_draws else None)
        keep, ph, nh, pr = self._fused_args(h, Register, "tx_frames")
        sm, sv = _imp_mode(Time_Delay, "tx_frames")
        cm, cv = _imp_mode(Freq_Shift, "tx_frames")
        L.check(self.lib.ofdm_tx_frames_ex(self.handle, ph, nh, float(SNR if SNR is not None else 0.0), int(SNR is not None),
                                           int(seed), int(frame0), n_frames, pr, sm, int(sv), cm, float(cv),
                                           int(bool(noise_first)), *ptrs, flags), "tx_frames")
        out = dict(rx=rx.t() if device is not None else rx.T, packed=packed)
        if want_bits:
            out["bits"] = bits
        if scr:
            out["sc_packed"] = scp
        if want_draws:
            out["Time_Delay"], out["Freq_Shift"] = sto, cfo
        return out

    def _fused_args(self, h, Register, what):
        cdt_np = np.complex128 if self.f64 else np.complex64
        hh = None
        if h is not None:
            hh = np.ascontiguousarray(np.asarray(h.cpu().numpy() if _is_torch(h) else h).ravel().astype(cdt_np))
        reg = None
        if Register is not None:
            reg = np.ascontiguousarray(np.asarray(Register).ravel().astype(np.uint8))
            if reg.size != 15:
                raise OfdmError(f"{what}: Register must have 15 entries")
        ph = hh.ctypes.data_as(C.c_void_p) if hh is not None else None
        pr = reg.ctypes.data_as(C.c_void_p) if reg is not None else None
        return (hh, reg), ph, 0 if hh is None else hh.size, pr

    @staticmethod
    def _fading_args(h, fading, what):
        """fading=(delays, powers) of a tap-delay line -> (kept arrays, delay pointer, power pointer, n_taps)."""
        if h is not None:
            raise OfdmError(f"{what}: give h= (one channel for every frame) or fading= (a channel per frame), not both")
        try:
            delays, powers = fading
        except (TypeError, ValueError):
            raise OfdmError(f"{what}: fading must be (delays, powers)") from None
        dl = np.asarray(delays).ravel()
        if dl.size and not np.all(dl == np.rint(dl)):
            raise OfdmError(f"{what}: fading delays must be whole samples")
        dl = np.ascontiguousarray(dl.astype(np.int32))
        pw = np.ascontiguousarray(np.asarray(powers, dtype=np.float64).ravel())
        if pw.size != dl.size:
            raise OfdmError(f"{what}: fading needs one power per delay")
        return (dl, pw), dl.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p), int(dl.size)

    def _outputs(self, device, *specs):
        """Row-major outputs of one plan call, one per (shape, numpy dtype) spec, None for an output not wanted: torch
        tensors on `device` (the call runs on its current stream) when it is given, numpy arrays on the default stream
        otherwise.  -> (arrays, their pointers, the call's flags)"""
        flags = L.OFDM_F64 if self.f64 else L.OFDM_F32
        if device is not None:
            dev = torch.device(device)
            arrs = [None if sp is None else torch.empty(sp[0], dtype=_torch_dtype(sp[1]), device=dev) for sp in specs]
            L.check(self.lib.ofdm_set_stream(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "set_stream")
            return arrs, [None if t is None else C.c_void_p(t.data_ptr()) for t in arrs], flags | L.OFDM_DEVICE
        L.check(self.lib.ofdm_set_stream(None), "set_stream")
        arrs = [None if sp is None else np.empty(sp[0], dtype=sp[1]) for sp in specs]
        return arrs, [None if x is None else x.ctypes.data_as(C.c_void_p) for x in arrs], flags

    @staticmethod
    def _points(SNRs, seeds, seed, what):
        """The SNR row of a sweep and one Philox key per point (`seed` for every point when `seeds` is None), as arrays (the
        caller holds them until the call has returned) and as the two pointers the C entries take."""
        snr = np.ascontiguousarray(np.asarray(SNRs, dtype=np.float64).ravel())
        sd = np.full(snr.size, int(seed), dtype=np.uint64) if seeds is None else \
            np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).ravel())
        if sd.size != snr.size:
            raise OfdmError(f"{what}: seeds must have one entry per SNR point")
        return snr, sd, snr.ctypes.data_as(C.c_void_p), sd.ctypes.data_as(C.c_void_p)

    def _sweep_channel(self, h, fading, Register, what):
        """The channel and the register of a BER sweep: fading=(delays, powers) or h (both: refused here), then Register ->
        (kept arrays, (h, h_len), (tap_delay, tap_power, n_taps), scr_reg15) as the C entries take them."""
        if fading is not None:
            keep_f, pdl, ppw, nt = self._fading_args(h, fading, what)
            keep, _, _, pr = self._fused_args(None, Register, what)
            return keep_f + keep, (None, 0), (pdl, ppw, nt), pr
        keep, ph, nh, pr = self._fused_args(h, Register, what)
        return keep, (ph, nh), (None, None, 0), pr

    @staticmethod
    def _density_args(density, what):
        """density=dict(bins=, half_width=, skip=0) of a sweep -> (bins, half_width, skip)."""
        try:
            extra = set(density) - {"bins", "half_width", "skip"}
            bins, half_width, skip = int(density["bins"]), float(density["half_width"]), int(density.get("skip", 0))
        except (TypeError, KeyError, ValueError, AttributeError):
            raise OfdmError(f"{what}: density must be dict(bins=, half_width=, skip=0)") from None
        if extra:
            raise OfdmError(f"{what}: unknown density keys {sorted(extra)}")
        return bins, half_width, skip

    def _density_outputs(self, device, n, bins):
        """The density grids [n, bins, bins] and dropped counters [n] of a sweep -> (their two pointers, the result entries:
        int64 views of the numpy arrays -- a count of 2^63 is out of reach -- the device tensors as they are)."""
        nb = bins if bins > 0 else 0                              # (a bad count is the library's refusal)
        (dens, drop), dptrs, _ = self._outputs(device, ((n, nb, nb), np.uint64), ((n,), np.uint64))
        if device is None:
            dens, drop = dens.view(np.int64), drop.view(np.int64)
        return dptrs, dict(density=dens, density_dropped=drop)

    def _study_args(self, what, SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift):
        """The generator arguments every study entry takes, as its C signature groups them -> (keep, n_points, chan = (h, h_len,
        tap_delay, tap_power, n_taps), imp = (sto_mode, sto_value, cfo_mode, cfo_value), scr_reg15, pts = (snr_db, seeds,
        n_points)).  keep: the arrays behind the pointers; the caller holds it until the call has returned."""
        snr, sd, psnr, psd = self._points(SNRs, seeds, seed, what)
        keep, ph, nh, pr = self._fused_args(h, Register, what)
        pdl, ppw, nt = None, None, 0
        if fading is not None:                                   # (with h too: the library's refusal)
            keep_f, pdl, ppw, nt = self._fading_args(None, fading, what)
            keep += keep_f
        sm, sv = _imp_mode(Time_Delay, what)
        cm, cv = _imp_mode(Freq_Shift, what)
        return keep + (snr, sd), snr.size, (ph, nh, pdl, ppw, nt), (sm, int(sv), cm, float(cv)), pr, (psnr, psd, snr.size)

    @staticmethod
    def _counts(device, count, *tables):
        """What a study's means are formed with -> (the counter `tables` as int64: views of the numpy uint64 arrays -- a count of
        2^63 is out of reach -- the device tensors as they are; `count` as a float64 divisor: a tensor on the device, so that the
        division is an IEEE division as numpy's, where a Python scalar would multiply by its reciprocal (None: no divisor is made,
        and on the device nothing is launched for it); the cast to float64)."""
        if device is None:
            return [a.view(np.int64) for a in tables], None if count is None else np.float64(count), lambda a: a.astype(np.float64)
        div = None if count is None else torch.full((1,), float(count), dtype=torch.float64, device=torch.device(device))
        return list(tables), div, lambda a: a.double()

    @staticmethod
    def _payload(device, payload_bits, payload_packed, what):
        """The caller's payload as the C entries take it: payload_bits (a 0 / 1 array or tensor of any length and shape, read
        in C order) packed MSB first, or payload_packed=(bytes, n_bits) as it is -> (the packed buffer: a torch uint8 tensor on
        `device` when it is given, a numpy array otherwise; its pointer; n_bits).  Packing is byte plumbing: numpy's packbits on
        the host, the same weights in torch for a CUDA tensor, which never leaves the device."""
        if (payload_bits is None) == (payload_packed is None):
            raise OfdmError(f"{what}: give payload_bits or payload_packed=(bytes, n_bits), not both")
        if payload_packed is not None:
            try:
                raw, n_bits = payload_packed
                n_bits = int(n_bits)
            except (TypeError, ValueError):
                raise OfdmError(f"{what}: payload_packed must be (bytes, n_bits)") from None
            if _is_torch(raw):
                buf = raw.contiguous().view(-1)
                if buf.dtype != torch.uint8:
                    raise OfdmError(f"{what}: payload_packed bytes must be uint8")
            elif isinstance(raw, (bytes, bytearray, memoryview)):
                buf = np.frombuffer(raw, dtype=np.uint8)
            else:
                buf = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).ravel())
            if 8 * int(buf.numel() if _is_torch(buf) else buf.size) < n_bits:
                raise OfdmError(f"{what}: payload_packed holds fewer than n_bits = {n_bits} bits")
        elif _is_torch(payload_bits) and payload_bits.is_cuda:
            b = (payload_bits.reshape(-1) != 0).to(torch.uint8)
            n_bits = int(b.numel())
            b = torch.nn.functional.pad(b, (0, (-n_bits) % 8)).view(-1, 8)
            w = torch.tensor([128, 64, 32, 16, 8, 4, 2, 1], dtype=torch.uint8, device=b.device)
            buf = (b * w).sum(dim=1).to(torch.uint8)
        else:
            b = np.asarray(payload_bits.numpy() if _is_torch(payload_bits) else payload_bits).ravel() != 0
            n_bits = int(b.size)
            buf = np.packbits(b)
        if (buf.numel() if _is_torch(buf) else buf.size) == 0:       # (no bits: a byte to point at, the count is the library's refusal)
            buf = np.zeros(1, np.uint8)
        if device is not None:
            buf = (buf if _is_torch(buf) else torch.from_numpy(np.array(buf))).to(torch.device(device)).contiguous()
            return buf, C.c_void_p(buf.data_ptr()), n_bits
        if _is_torch(buf):
            buf = buf.cpu().numpy()
        buf = np.ascontiguousarray(buf)
        return buf, buf.ctypes.data_as(C.c_void_p), n_bits

    def tx_frames_fused(self, n_frames, h=None, SNR=20.0, seed=1, frame0=0, device=None, Register=None, Time_Delay=None,
                        Freq_Shift=None, want_draws=False, fading=None, want_taps=False, payload_bits=None, payload_frame0=0,
                        payload_packed=None):
        """Reference-order frames in three sample passes (ofdm_tx_frames_fused): payload -> [Scrambler(Register, .) per
        frame] -> mapping -> OFDM_map_carriers -> OFDM_modulator -> Noise(SNR) -> conv(h) truncated
        (T5/Main_model_Task_5.m:50-127, T5/Task5_part2.m:134,:152).  The draws of tx_frames(noise_first=True): the same
        frames up to rounding.  h=None: no channel.
        Time_Delay / Freq_Shift (as in tx_frames: None = off, a number = that value for every frame, "random" = the
        per-frame draw of T4/Main_model_Task_4.m:101-110) add add_STO -> add_CFO between Noise and conv
        (ofdm_tx_frames_fused_ex, T4:94-110); want_draws returns the per-frame values.
        Returns dict(rx=[frame_samples, n_frames], packed=[n_frames, frame_bytes] (the payload bits)
        (+ sc_packed = the scrambled bits when Register is given) (+ Time_Delay [n_frames] int64, Freq_Shift [n_frames]
        float64 with want_draws)); torch CUDA tensors when `device` is given.
        fading=(delays, powers) (ofdm_tx_frames_fading; not with h): a channel per frame on one
        tap-delay line -- 0-based distinct sample delays and linear powers (drivers.common.fading_profile gives the 3GPP
        ones) -- the stand-in for lteFadingChannel of T5/Task5_part2.m:148-155: tap t of frame f is sqrt(powers[t] /
        sum(powers)) e^{2 pi i u} with u from Philox counter (t, 0, frame0 + f, 3), key `seed`.  want_taps adds
        taps=[n_frames, n_taps] complex128, those amplitudes.  With Time_Delay / Freq_Shift / want_draws too
        (ofdm_tx_frames_fading_ex): Noise -> add_STO -> add_CFO -> conv with the frame's own taps, the two per-frame draws
        independent of each other.
        The C entry: ofdm_tx_frames_fused, with fading ofdm_tx_frames_fading; given Time_Delay, Freq_Shift or want_draws their
        _ex forms.  The plain entries launch no STO / CFO draw kernel and the channel pass without impairments.
        payload_bits (a 0 / 1 array or torch tensor of any length) or payload_packed=(bytes, n_bits) (packed MSB first, as
        `packed` is) replace the payload draw (ofdm_tx_frames_payload): frame f carries the stream bits (payload_frame0 + f)
        frame_bits .. + frame_bits - 1, zeros at and beyond the stream's end (display_pic.m:5-6); the noise, STO / CFO and
        fading draws stay those of (seed, frame0 + f), and for the Philox bits of (seed, frame0 + f) every output is the one
        without a payload, bit for bit.  With neither, the function is what it was."""
        n_frames = int(n_frames)
        given = payload_bits is not None or payload_packed is not None
        fade = fading is not None
        if fade:
            keep_f, pdl, ppw, nt = self._fading_args(h, fading, "tx_frames_fused")
            chan, name = (pdl, ppw, nt), "tx_frames_fading"
        elif want_taps:
            raise OfdmError("tx_frames_fused: want_taps needs fading")
        ex = Time_Delay is not None or Freq_Shift is not None or want_draws
        scr = Register is not None
        (rx, packed, scp, taps, sto, cfo), ptrs, flags = self._outputs(
            device, ((n_frames, self.frame_samples), np.complex128 if self.f64 else np.complex64),
            ((n_frames, self.frame_bytes), np.uint8), ((n_frames, self.frame_bytes), np.uint8) if scr else None,
            ((n_frames, nt), np.complex128) if fade and want_taps else None, ((n_frames,), np.int64) if want_draws else None,
            ((n_frames,), np.float64) if want_draws else None)
        keep, ph, nh, pr = self._fused_args(None if fade else h, Register, "tx_frames_fused")
        if not fade:
            chan, name = (ph, nh), "tx_frames_fused"
        p_bits, p_taps, p_draws = ptrs[:3], ptrs[3:4] if fade else [], ptrs[4:]
        if given:
            pbuf, pp, n_bits = self._payload(device, payload_bits, payload_packed, "tx_frames_fused")
            sm, sv = _imp_mode(Time_Delay, "tx_frames_fused")
            cm, cv = _imp_mode(Freq_Shift, "tx_frames_fused")
            ch5 = (None, 0, *chan) if fade else (*chan, None, None, 0)
            L.check(self.lib.ofdm_tx_frames_payload(self.handle, pp, n_bits, int(payload_frame0), *ch5, float(SNR), int(seed),
                                                    int(frame0), n_frames, pr, sm, int(sv), cm, float(cv), *ptrs, flags),
                    "tx_frames_payload")
        elif ex:
            sm, sv = _imp_mode(Time_Delay, "tx_frames_fused")
            cm, cv = _imp_mode(Freq_Shift, "tx_frames_fused")
            L.check(getattr(self.lib, f"ofdm_{name}_ex")(self.handle, *chan, float(SNR), int(seed), int(frame0), n_frames, pr,
                                                         sm, int(sv), cm, float(cv), *p_bits, *p_taps, *p_draws, flags),
                    f"{name}_ex")
        else:
            L.check(getattr(self.lib, f"ofdm_{name}")(self.handle, *chan, float(SNR), int(seed), int(frame0), n_frames, pr,
                                                      *p_bits, *p_taps, flags), name)
        out = dict(rx=rx.t() if device is not None else rx.T, packed=packed)
        if scr:
            out["sc_packed"] = scp
        if want_taps:
            out["taps"] = taps
        if want_draws:
            out["Time_Delay"], out["Freq_Shift"] = sto, cfo
        return out

    def papr_study(self, n_signals, frames_per_signal=1, seed=1, frame0=0, Register=None, payload_bits=None, window=None,
                   bins=dict(n=600, lo=0.0, hi=30.0), device=None, want_tx=False, max_frames_per_chunk=0):
        """The PAPR / CCDF study of T2/Main_model_Task_2.m:69-97 over n_signals signals in one device-resident call
        (ofdm_papr_study).  A signal is frames_per_signal consecutive frames of this plan, concatenated (T2:64-68): payload ->
        [Scrambler(Register, .) per frame, T2:36-51] -> mapping -> OFDM_map_carriers -> OFDM_modulator, the frames of
        tx_frames_fused(seed, frame0) before Noise.  payload_bits [n_signals * frames_per_signal, frame_bits] (0 / 1) replace the
        Philox payload.  Every window of `window` samples (default Nfft; a power of two 256 .. 8192) of every signal is counted by
        its calculate_window_PAPR value on the grid bins=dict(n=, lo=, hi=) in dB.
        Returns dict(hist=[n] int64 (bin i: lo + i (hi - lo) / n <= v < the next edge), below, above (v >= hi), dropped (NaN: an
        all-zero window), windows = the windows counted = hist.sum() + below + above + dropped, edges=[n + 1],
        CCDF=[n + 1] = the share of the non-NaN windows with v >= edges[i] (calculateCCDF.m:2-6 on the grid), peak=[n_signals]
        max |x|^2, power_sum=[n_signals] sum |x|^2, PAPR_dB=[n_signals] = calculatePAPR of each signal (T2:72-73)
        (+ tx=[frames_per_signal * frame_samples, n_signals] with want_tx)); torch tensors on `device` (no host synchronisation;
        below / above / dropped / windows then 0-d tensors) when it is given, numpy arrays and ints otherwise.  No output depends
        on max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned workspace, rounded down to whole signals)."""
        try:
            extra = set(bins) - {"n", "lo", "hi"}
            nb, lo, hi = int(bins["n"]), float(bins["lo"]), float(bins["hi"])
        except (TypeError, KeyError, ValueError, AttributeError):
            raise OfdmError("papr_study: bins must be dict(n=, lo=, hi=)") from None
        if extra:
            raise OfdmError(f"papr_study: unknown bins keys {sorted(extra)}")
        ns, fps = int(n_signals), int(frames_per_signal)
        window = self.Nfft if window is None else int(window)
        n_alloc, f_alloc, b_alloc = max(ns, 0), max(fps, 0), min(max(nb, 0), 4096)    # (a bad count is the library's refusal)
        (hist, tails, sig, tx), ptrs, flags = self._outputs(
            device, ((b_alloc,), np.uint64), ((3,), np.uint64), ((n_alloc, 2), np.float64),
            ((n_alloc, f_alloc * self.frame_samples), np.complex128 if self.f64 else np.complex64) if want_tx else None)
        keep, _, _, pr = self._fused_args(None, Register, "papr_study")
        pb = None
        if payload_bits is not None:
            want = n_alloc * f_alloc * self.frame_bits
            if int(np.prod(tuple(payload_bits.shape))) != want:
                raise OfdmError(f"papr_study: payload_bits must hold n_signals * frames_per_signal * frame_bits = {want} bits")
            if device is not None:
                bt = payload_bits if _is_torch(payload_bits) else torch.as_tensor(np.asarray(payload_bits))
                bt = (bt != 0).to(device=torch.device(device), dtype=torch.uint8).contiguous()
                pb = C.c_void_p(bt.data_ptr())
            else:
                bt = np.ascontiguousarray(np.asarray(payload_bits.cpu().numpy() if _is_torch(payload_bits) else payload_bits) != 0,
                                          dtype=np.uint8)
                pb = bt.ctypes.data_as(C.c_void_p)
        L.check(self.lib.ofdm_papr_study(self.handle, int(seed), int(frame0), ns, fps, pr, pb, window, nb, lo, hi,
                                         int(max_frames_per_chunk), *ptrs, flags), "papr_study")
        n_sig = fps * self.frame_samples
        if device is not None:
            xp, edges = torch, torch.from_numpy(np.linspace(lo, hi, nb + 1)).to(hist.device)
            below, above, dropped = tails[0], tails[1], tails[2]
            counted = hist.sum()
            tail_cum = torch.flip(torch.cumsum(torch.flip(hist, (0,)), 0), (0,))
            exceed = (torch.cat([tail_cum, torch.zeros(1, dtype=hist.dtype, device=hist.device)]) + above).double()
        else:
            hist, tails = hist.view(np.int64), tails.view(np.int64)          # int64 views: a count of 2^63 is out of reach
            xp, edges = np, np.linspace(lo, hi, nb + 1)
            below, above, dropped = int(tails[0]), int(tails[1]), int(tails[2])
            counted = int(hist.sum())
            exceed = (np.concatenate([np.cumsum(hist[::-1])[::-1], [0]]) + above).astype(np.float64)
        valid = counted + below + above
        with np.errstate(divide="ignore", invalid="ignore"):                 # no window counted: NaN, like ecdf of nothing
            ccdf = exceed / (valid.double() if device is not None else np.float64(valid))
        peak, power_sum = sig[:, 0], sig[:, 1]
        out = dict(hist=hist, below=below, above=above, dropped=dropped, windows=valid + dropped, edges=edges,
                   CCDF=ccdf, peak=peak, power_sum=power_sum,
                   PAPR_dB=10.0 * xp.log10(peak / (power_sum / n_sig)))      # calculatePAPR.m:4-10
        if want_tx:
            out["tx"] = tx.t() if device is not None else tx.T
        return out

    def spectrum_study(self, SNRs, frames_per_point, h=None, fading=None, Time_Delay=None, Freq_Shift=None, seeds=None, seed=1,
                       frame0=0, Register=None, first=None, n_windows=1, device=None, want_peak=False, want_frame_power=False,
                       max_frames_per_chunk=0):
        """The averaged periodogram of a sweep in one device-resident call (ofdm_spectrum_study): for every SNR of `SNRs` the frames
        frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay, Freq_Shift),
        bit for bit, and of each frame the power row of rx_spectrum(first, n_windows): per bin the sum over the windows
        first + w (Nfft + T_guard) .. + Nfft - 1 of |fft|^2, in double.  first defaults to T_guard (the
        abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard))) of T3/Main_model_Task_3.m:138).  No receiver runs.
        Returns dict(power_sums=[n_points, Nfft] float64, each point's power rows summed in frame order; mean_power = power_sums /
        (frames_per_point * n_windows); amp_rms = sqrt(mean_power) (+ peak=[n_points, Nfft], the largest |fft|^2 of any frame and
        window, with want_peak) (+ frame_power=[n_points, frames_per_point, Nfft] with want_frame_power)); torch tensors on
        `device` (no host synchronisation) when it is given, numpy arrays otherwise.  No output depends on max_frames_per_chunk
        (> 0: the frames of a chunk of the plan-owned workspace)."""
        keep, n, chan, imp, pr, pts = self._study_args("spectrum_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp = int(frames_per_point)
        first = self.T_guard if first is None else int(first)
        nw = int(n_windows)
        (sums, peak, fp), ptrs, flags = self._outputs(
            device, ((n, self.Nfft), np.float64), ((n, self.Nfft), np.float64) if want_peak else None,
            ((n, max(fpp, 0), self.Nfft), np.float64) if want_frame_power else None)
        L.check(self.lib.ofdm_spectrum_study(self.handle, *chan, *imp, pr, *pts, fpp, int(frame0), int(max_frames_per_chunk), first,
                                             nw, *ptrs, flags), "spectrum_study")
        _, count, _ = self._counts(device, fpp * nw)
        with np.errstate(divide="ignore", invalid="ignore"):     # no frames: NaN, the mean of nothing
            mean = sums / count
        out = dict(power_sums=sums, mean_power=mean, amp_rms=mean.sqrt() if device is not None else np.sqrt(mean))
        if want_peak:
            out["peak"] = peak
        if want_frame_power:
            out["frame_power"] = fp
        return out

    def sync_study(self, SNRs, frames_per_point, h=None, fading=None, Time_Delay=None, Freq_Shift=None, width=None, seeds=None,
                   seed=1, frame0=0, Register=None, device=None, want_peak=False, want_frames=False, max_frames_per_chunk=0):
        """The coarse synchroniser's pictures of a sweep in one device-resident call (ofdm_sync_study): for every SNR of `SNRs` the
        frames frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay,
        Freq_Shift), bit for bit, and of each frame the outputs of rx_acf(width): abs(AutoCorr) of AutoCorrFunction(frame, width,
        Nfft) (T4/Main_model_Task_4.m:282-287, figures 6-10 of the Task-4 report), TgPosition and FreqOffset.  width defaults to
        T_guard (T4:278).  No receiver runs behind the autocorrelation, and the integer offset of remove_IFO is out of scope.
        Returns dict(acf_sums=[n_points, n_out] float64, n_out = frame_samples - width - Nfft: each point's amp rows summed per lag in
        frame order, the values that are not finite (the zero tail of add_STO: 0 / 0) left out and counted in acf_dropped=[n_points,
        n_out] int64; mean_acf = acf_sums / (frames_per_point - acf_dropped); tg_hist=[n_points, n_out] int64, the frames by
        TgPosition - 1 (the catch branch's 65 in bin 64; with n_out <= 64 only in fallback); fallback=[n_points] int64, the frames
        that took the catch branch; phase_hist=[n_points, Nfft + T_guard] int64, the frames by (TgPosition - 1 + the frame's own
        Time_Delay) mod (Nfft + T_guard): sharp whatever the delay; ffo_err=[n_points, 2] float64 = {sum |e|, sum e^2} of the wrapped
        fractional error e of FreqOffset against the frame's own Freq_Shift (T4:113-135), mean_abs_ffo_err = ffo_err[:, 0] /
        frames_per_point (+ acf_peak=[n_points, n_out], fmax over the frames, with want_peak) (+ tg_position, status, freq_offset =
        [n_points, frames_per_point] with want_frames)); torch tensors on `device` (no host synchronisation) when it is given,
        numpy arrays otherwise.  No output depends on max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned
        workspace)."""
        keep, n, chan, imp, pr, pts = self._study_args("sync_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp = int(frames_per_point)
        W = self.T_guard if width is None else int(width)
        n_out = max(self.frame_samples - W - self.Nfft, 0) if 1 <= W <= 1024 else 0     # (a bad width is the library's refusal)
        fa = max(fpp, 0)
        (sums, drop, peak, tgh, fall, ph, ffo, ftg, fst, ffo_f), ptrs, flags = self._outputs(
            device, ((n, n_out), np.float64), ((n, n_out), np.uint64), ((n, n_out), np.float64) if want_peak else None,
            ((n, n_out), np.uint64), ((n,), np.uint64), ((n, self.Nfft + self.T_guard), np.uint64), ((n, 2), np.float64),
            ((n, fa), np.int64) if want_frames else None, ((n, fa), np.int32) if want_frames else None,
            ((n, fa), np.float64) if want_frames else None)
        L.check(self.lib.ofdm_sync_study(self.handle, *chan, *imp, pr, *pts, fpp, int(frame0), int(max_frames_per_chunk), W, *ptrs,
                                         flags), "sync_study")
        (drop, tgh, fall, ph), count, f64 = self._counts(device, fpp, drop, tgh, fall, ph)
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame added: NaN, the mean of nothing
            mean = sums / f64(fpp - drop)
            mae = ffo[:, 0] / count
        out = dict(acf_sums=sums, acf_dropped=drop, mean_acf=mean, tg_hist=tgh, fallback=fall, phase_hist=ph, ffo_err=ffo,
                   mean_abs_ffo_err=mae)
        if want_peak:
            out["acf_peak"] = peak
        if want_frames:
            out.update(tg_position=ftg, status=fst, freq_offset=ffo_f)
        return out

    def fine_study(self, SNRs, frames_per_point, h=None, fading=None, Time_Delay=None, Freq_Shift=None, time_desync=1, freq_desync=0,
                   variant="T4", bins=None, seeds=None, seed=1, frame0=0, Register=None, device=None, want_frames=False,
                   max_frames_per_chunk=0):
        """The fine synchroniser's pictures of a sweep in one device-resident call (ofdm_fine_study): for every SNR of `SNRs` the
        frames frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay,
        Freq_Shift), bit for bit, through the front end of rx_chain_task4(time_desync, freq_desync) exactly as that receiver runs
        it -- AutoCorrFunction(Rx, T_guard, Nfft), the two add_STO, with freq_desync add_CFO(-FreqOffset) and remove_IFO, the
        demodulator (T4/Main_model_Task_4.m:278-310) -- and of each frame the outputs of rx_fine(variant, time_desync) on the
        pilot rows.  Nothing behind fine_sync's estimates runs.  bins = dict(n, lo, hi) (default 64 bins on [-4, 4)) is the
        histogram of the timing error in samples, e = tau Nfft + phi_s + 1 with phi = (TgPosition - 1 + Time_Delay) mod
        (Nfft + T_guard) wrapped into (-(Nfft + T_guard) / 2, (Nfft + T_guard) / 2]: 0 where fine_sync measures what the coarse
        stage left.
        Returns dict(tau_curve_sums=[n_points, L] float64, taus(i) summed in frame order, the values that are not finite counted
        in curve_dropped=[n_points, L] int64; keep_counts=[n_points, L] int64, the frames whose entry passed the 1e-3 mask
        (keep_rate = keep_counts / frames_per_point); tau_hist=[n_points, bins.n], tau_below, tau_above, tau_nan=[n_points] int64
        (their sum is frames_per_point; tau_nan: the frames where tau = mean([])); edges=[bins.n + 1]; tau_err=[n_points, 2]
        float64 = {sum |e|, sum e^2} over the finite e, mean_abs_err = tau_err[:, 0] / (frames_per_point - tau_nan);
        phase_sums=[n_points, 2] float64 = {sum phase, sum phase^2} over the finite values, phase_nan=[n_points] int64;
        used_sums=[n_points] int64 = sum n_used; tg_hist=[n_points, Nfft + T_guard] int64, the frames by phi
        (+ frame_tau, frame_phase float64, frame_n_used int32, frame_tg_position int64, frame_status int32, frame_time_delay int64 =
        [n_points, frames_per_point] with want_frames)); torch tensors on `device` (no host synchronisation) when it is given,
        numpy arrays otherwise.  No output depends on max_frames_per_chunk (> 0: the frames of a chunk)."""
        if variant not in _FINE_VARIANTS:
            raise OfdmError("fine_study: variant must be 'T4' or 'T5'")
        bins = dict(n=64, lo=-4.0, hi=4.0) if bins is None else bins
        try:
            bn, blo, bhi = int(bins["n"]), float(bins["lo"]), float(bins["hi"])
        except (TypeError, KeyError, ValueError):
            raise OfdmError("fine_study: bins must be dict(n=, lo=, hi=)") from None
        keep, n, chan, imp, pr, pts = self._study_args("fine_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp = int(frames_per_point)
        Lt = _fine_len(self.n_pilots, self.N_symb, variant)
        fa, nb = max(fpp, 0), max(bn, 0)
        fr = lambda dt: ((n, fa), dt) if want_frames else None
        (sums, drop, keepc, hist, below, above, tnan, terr, psum, pnan, used, tgh, ftau, fph, fnu, ftg, fst, ftd), ptrs, flags = \
            self._outputs(device, ((n, Lt), np.float64), ((n, Lt), np.uint64), ((n, Lt), np.uint64), ((n, nb), np.uint64),
                          ((n,), np.uint64), ((n,), np.uint64), ((n,), np.uint64), ((n, 2), np.float64), ((n, 2), np.float64),
                          ((n,), np.uint64), ((n,), np.uint64), ((n, self.Nfft + self.T_guard), np.uint64), fr(np.float64),
                          fr(np.float64), fr(np.int32), fr(np.int64), fr(np.int32), fr(np.int64))
        L.check(self.lib.ofdm_fine_study(self.handle, *chan, *imp, int(bool(time_desync)), int(bool(freq_desync)),
                                         _FINE_VARIANTS[variant], pr, *pts, fpp, int(frame0), int(max_frames_per_chunk), bn, blo,
                                         bhi, *ptrs, flags), "fine_study")
        (drop, keepc, hist, below, above, tnan, pnan, used, tgh), count, f64 = self._counts(
            device, fpp, drop, keepc, hist, below, above, tnan, pnan, used, tgh)
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame counted: NaN, the mean of nothing
            rate = f64(keepc) / count
            mae = terr[:, 0] / f64(fpp - tnan)
        edges = np.linspace(blo, bhi, nb + 1)
        if device is not None:                                   # like every other output (and papr_study's edges)
            edges = torch.from_numpy(edges).to(sums.device)
        out = dict(tau_curve_sums=sums, curve_dropped=drop, keep_counts=keepc, keep_rate=rate, tau_hist=hist, tau_below=below,
                   tau_above=above, tau_nan=tnan, edges=edges, tau_err=terr, mean_abs_err=mae,
                   phase_sums=psum, phase_nan=pnan, used_sums=used, tg_hist=tgh)
        if want_frames:
            out.update(frame_tau=ftau, frame_phase=fph, frame_n_used=fnu, frame_tg_position=ftg, frame_status=fst,
                       frame_time_delay=ftd)
        return out

    def ifo_study(self, SNRs, frames_per_point, h=None, fading=None, Time_Delay=None, Freq_Shift=None, stage="receiver", time_desync=1,
                  err_span=32, seeds=None, seed=1, frame0=0, Register=None, device=None, want_frames=False, max_frames_per_chunk=0):
        """remove_IFO's pictures of a sweep in one device-resident call (ofdm_ifo_study): for every SNR of `SNRs` the frames
        frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay, Freq_Shift),
        bit for bit, and of each frame the outputs of rx_ifo(stage, time_desync): the spectrum abs(fft(rx_signal(Nfft+1 : 2*Nfft)))
        of T4/remove_IFO.m:5, IFO = inds(1) - 1 and the bins above 0.77.  stage="raw": remove_IFO on the received frame with
        AutoCorrFunction beside it, the study of T4/Main_model_Task_4.m:113-135 (figure 13b of the Task-4 report);
        stage="receiver": behind the receiver's two add_STO (with time_desync) and add_CFO(-FreqOffset), T4:278-303.  Nothing
        behind remove_IFO's pick runs.
        Returns dict(spec_sums=[n_points, Nfft] float64, each point's amp rows summed per bin in frame order, the values that are
        not finite counted in spec_dropped=[n_points, Nfft] int64; mean_spec = spec_sums / (frames_per_point - spec_dropped);
        above_counts=[n_points, Nfft] int64, the frames whose bin exceeds 0.77; ifo_hist=[n_points, Nfft] int64, the frames with
        a line by IFO; no_line=[n_points] int64, the frames without one (status -1), no_line_rate = no_line / frames_per_point;
        err_hist=[n_points, 2 err_span + 1], err_below, err_above=[n_points] int64, the frames with a line by IFO -
        rint(Freq_Shift) against the frame's own draw (bin err_span is 0); hit=[n_points] int64, the frames with error 0,
        hit_rate = hit / frames_per_point; cfo_err=[n_points, 2] float64 = {sum |e|, sum e^2} of e = FreqOffset + IFO -
        Freq_Shift over the frames with a line, mean_abs_cfo_err = cfo_err[:, 0] / (frames_per_point - no_line) (the y axis of
        T4:130); fallback=[n_points] int64, the frames whose status is 1 (AutoCorrFunction's catch branch)
        (+ ifo, status, n_above int32, tg_position int64, freq_offset float64 = [n_points, frames_per_point] with want_frames));
        torch tensors on `device` (no host synchronisation) when it is given, numpy arrays otherwise.  No output depends on
        max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned workspace)."""
        keep, n, chan, imp, pr, pts = self._study_args("ifo_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp, span = int(frames_per_point), int(err_span)
        fa, ne = max(fpp, 0), 2 * span + 1 if 1 <= span <= 4096 else 0   # (a bad span is the library's refusal)
        fr = lambda dt: ((n, fa), dt) if want_frames else None
        N = self.Nfft
        (sums, drop, above, hist, none, ehist, ebelow, eabove, hit, cerr, fall, fifo, fst, fna, ftg, ffo), ptrs, flags = \
            self._outputs(device, ((n, N), np.float64), ((n, N), np.uint64), ((n, N), np.uint64), ((n, N), np.uint64),
                          ((n,), np.uint64), ((n, ne), np.uint64), ((n,), np.uint64), ((n,), np.uint64), ((n,), np.uint64),
                          ((n, 2), np.float64), ((n,), np.uint64), fr(np.int32), fr(np.int32), fr(np.int32), fr(np.int64),
                          fr(np.float64))
        L.check(self.lib.ofdm_ifo_study(self.handle, *chan, *imp, _ifo_stage(stage, "ifo_study"), int(time_desync), pr, *pts, fpp,
                                        int(frame0), int(max_frames_per_chunk), span, *ptrs, flags), "ifo_study")
        (drop, above, hist, none, ehist, ebelow, eabove, hit, fall), count, f64 = self._counts(
            device, fpp, drop, above, hist, none, ehist, ebelow, eabove, hit, fall)
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame counted: NaN, the mean of nothing
            mean = sums / f64(fpp - drop)
            hit_rate, none_rate = f64(hit) / count, f64(none) / count
            mae = cerr[:, 0] / f64(fpp - none)
        out = dict(spec_sums=sums, spec_dropped=drop, mean_spec=mean, above_counts=above, ifo_hist=hist, no_line=none,
                   no_line_rate=none_rate, err_hist=ehist, err_below=ebelow, err_above=eabove, hit=hit, hit_rate=hit_rate,
                   cfo_err=cerr, mean_abs_cfo_err=mae, fallback=fall)
        if want_frames:
            out.update(ifo=fifo, status=fst, n_above=fna, tg_position=ftg, freq_offset=ffo)
        return out

    def channel_study(self, SNRs, frames_per_point, h=None, fading=None, Time_Delay=None, Freq_Shift=None, time_desync=0,
                      freq_desync=0, bins=dict(n=60, lo=-50.0, hi=10.0), seeds=None, seed=1, frame0=0, Register=None, device=None,
                      want_frame_nmse=False, max_frames_per_chunk=0):
        """estimate_channel's picture of a sweep in one device-resident call (ofdm_hest_study): figure 21 of the Task-4 report
        (T4/Main_model_Task_4.m:318-332) -- |H_freq|, the stems |Hest_at_pilots| and the dashed |H_est| over the carrier index --
        with the error of the estimate per carrier, per pilot and per frame.  For every SNR of `SNRs` the frames frame0 .. frame0 +
        frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay, Freq_Shift), bit for bit, and of
        each frame what rx_hest(time_desync, freq_desync) returns; nothing behind estimate_channel runs.  The true channel is
        H_f(k) = sum_t a_t e^{-2 pi i d_t k / Nfft} in float64 from the nonzero taps of h (none: one unit tap) or the frame's drawn
        amplitudes.  bins = dict(n, lo, hi): the histogram of the frames by 10 log10(frame_nmse / N_carrier) in dB.
        Returns dict(est_amp_sums, true_amp_sums, err_sums, amp_err_sums=[n_points, N_carrier] float64: sum_f |H_est_f(k)|,
        sum_f |H_f(k)|, sum_f |H_f(k) - H_est_f(k)|^2, sum_f (|H_est_f(k)| - |H_f(k)|)^2 in frame order, a frame whose H_est_f(k) is
        not finite left out of all four and counted in dropped=[n_points, N_carrier] int64; mean_est_amp, mean_true_amp = the two
        sums / (frames_per_point - dropped), the curves of figure 21; nmse_profile = err_sums / (frames_per_point - dropped);
        pilot_amp_sums (the stems), pilot_err_sums=[n_points, Np] float64 = sum_f |H_f(pilotCarriers(i)) - Hest_at_pilots_f(i)|^2,
        the error before interpolation, pilot_dropped=[n_points, Np] int64; nmse_sums=[n_points] float64, bit for bit those of
        ber_sweep_task4(mp_desync=1, want_nmse=True) for the same generator arguments and flags, NMSE = nmse_sums /
        (frames_per_point * N_carrier); amp_nmse_sums, amp_NMSE: the same of (|H_est| - |H|)^2, which does not see the ramp
        fine_sync removes; nmse_hist=[n_points, bins.n], nmse_below, nmse_above, nmse_nan=[n_points] int64 (their sum is
        frames_per_point), edges=[bins.n + 1] in dB and thresholds=[bins.n + 1] = N_carrier 10^(edges / 10), the table the frames
        were compared against (numpy, made on the host); status_counts=[n_points, 4] int64, the frames with status 0, 1, -1, -2
        (+ frame_nmse, frame_amp_nmse=[n_points, frames_per_point] float64 with want_frame_nmse)); torch tensors on `device` (no
        host synchronisation) when it is given, numpy arrays otherwise.  No output depends on max_frames_per_chunk (> 0: the frames
        of a chunk of the plan-owned workspace)."""
        try:
            extra = set(bins) - {"n", "lo", "hi"}
            bn, blo, bhi = int(bins["n"]), float(bins["lo"]), float(bins["hi"])
        except (TypeError, KeyError, ValueError):
            raise OfdmError("channel_study: bins must be dict(n=, lo=, hi=)") from None
        if extra:
            raise OfdmError(f"channel_study: unknown bins keys {sorted(extra)}")
        keep, n, chan, imp, pr, pts = self._study_args("channel_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp = int(frames_per_point)
        fa, nb = max(fpp, 0), bn if 1 <= bn <= 4096 else 0       # (a bad count is the library's refusal)
        nc, npil = self.N_carrier, self.n_pilots
        fr = ((n, fa), np.float64) if want_frame_nmse else None
        (esum, tsum, err, aerr, drop, pamp, perr, pdrop, ns, ans, fn, fan, hist, below, above, hnan, stc), ptrs, flags = \
            self._outputs(device, ((n, nc), np.float64), ((n, nc), np.float64), ((n, nc), np.float64), ((n, nc), np.float64),
                          ((n, nc), np.uint64), ((n, npil), np.float64), ((n, npil), np.float64), ((n, npil), np.uint64),
                          ((n,), np.float64), ((n,), np.float64), fr, fr, ((n, nb), np.uint64), ((n,), np.uint64),
                          ((n,), np.uint64), ((n,), np.uint64), ((n, 4), np.uint64))
        thr = np.zeros(nb + 1, np.float64)
        L.check(self.lib.ofdm_hest_study(self.handle, *chan, *imp, int(time_desync), int(freq_desync), pr, *pts, fpp, int(frame0),
                                         int(max_frames_per_chunk), bn, blo, bhi, *ptrs, thr.ctypes.data_as(C.c_void_p), flags),
                "hest_study")
        (drop, pdrop, hist, below, above, hnan, stc), _, f64 = self._counts(device, None, drop, pdrop, hist, below, above, hnan, stc)
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame counted: NaN, the mean of nothing
            kept = f64(fpp - drop)
            mean_est, mean_true, profile = esum / kept, tsum / kept, err / kept
            nmse, amp_nmse = ns / float(fpp * nc), ans / float(fpp * nc)
        edges = np.linspace(blo, bhi, nb + 1)
        out = dict(est_amp_sums=esum, true_amp_sums=tsum, err_sums=err, amp_err_sums=aerr, dropped=drop, mean_est_amp=mean_est,
                   mean_true_amp=mean_true, nmse_profile=profile, pilot_amp_sums=pamp, pilot_err_sums=perr, pilot_dropped=pdrop,
                   nmse_sums=ns, NMSE=nmse, amp_nmse_sums=ans, amp_NMSE=amp_nmse, nmse_hist=hist, nmse_below=below,
                   nmse_above=above, nmse_nan=hnan, edges=edges, thresholds=thr, status_counts=stc)
        if want_frame_nmse:
            out.update(frame_nmse=fn, frame_amp_nmse=fan)
        return out

    def error_study(self, SNRs, frames_per_point, receiver="task5", h=None, fading=None, Time_Delay=None, Freq_Shift=None,
                    time_desync=0, freq_desync=0, mp_desync=1, side="payload", gap_bins=64, want_map=False, want_frames=False,
                    seeds=None, seed=1, frame0=0, Register=None, device=None, max_frames_per_chunk=0):
        """Where a sweep point's bit errors sit, in one device-resident call (ofdm_error_study).  For every SNR of `SNRs` the frames
        frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h or fading, SNR, seeds[p], Register, Time_Delay, Freq_Shift), bit
        for bit, decoded as the matching sweep decodes them -- receiver="task5": rx_chain_task5 as in ber_sweep (the plan's route,
        its MMSE / mmse-ls / OMP-route modes; no Time_Delay / Freq_Shift, time_desync = freq_desync = 0, mp_desync = 1);
        receiver="task4": rx_chain_task4(time_desync, freq_desync, mp_desync) as in ber_sweep_task4 -- and the tables of
        bit_error_profile over each point's decisions.  The refusals of those sweeps apply in their own words.
        side="payload": what the receiver returns against the payload bits; `errors` is then ber_sweep(...)["errors"] /
        ber_sweep_task4(...)["errors"] for the same arguments, bit for bit.  side="channel": the decisions in front of the
        DeScrambler against the scrambled bits (sc_packed of tx_frames_fused): carrier, symbol and label then mean what they say,
        where the self-synchronising DeScrambler (T5/DeScrambler.m:8-13) turns every channel error into payload errors at i, i + 13
        and i + 14.  The plan's DeScrambler is masked inside the call and is as it was afterwards; without Register the two sides
        are the same bits.
        Returns the dict of bit_error_profile with a leading n_points on every table (frame_errors=[n_points, frames_per_point],
        map=[n_points, N_symb, nd]); torch tensors on `device` (no host synchronisation) when it is given, numpy arrays otherwise.
        No output depends on max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned workspace)."""
        try:
            rcv = {"task5": 5, "task4": 4, 5: 5, 4: 4}[receiver]
            sd_ = {"payload": 0, "channel": 1}[side]
        except (KeyError, TypeError):
            raise OfdmError('error_study: receiver must be "task5" or "task4", side "payload" or "channel"') from None
        keep, n, chan, imp, pr, pts = self._study_args("error_study", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        fpp, gb = int(frames_per_point), int(gap_bins)
        arrs, ptrs, flags = self._outputs(device, *_error_specs(self, n, max(fpp, 0), gb, want_frames, want_map))
        L.check(self.lib.ofdm_error_study(self.handle, rcv, *chan, *imp, int(time_desync), int(freq_desync), int(mp_desync), *pts, fpp,
                                          int(frame0), pr, sd_, gb, int(max_frames_per_chunk), *ptrs, flags), "error_study")
        return _error_result(self, device is not None, max(fpp, 0), arrs)

    def transport(self, payload_bits=None, SNRs=(20.0,), repeats=1, receiver="task5", h=None, fading=None, Time_Delay=None,
                  Freq_Shift=None, time_desync=0, freq_desync=0, mp_desync=1, seeds=None, seed=1, frame0=0, Register=None,
                  device=None, want_decoded=True, want_ones=False, want_frames=False, max_frames_per_chunk=0, payload_packed=None):
        """The caller's bits through the generator and a receiver and back as one stream, in one device-resident call
        (ofdm_payload_transport): what every driver of the reference does first (file_reader.m -> the chain -> DeScrambler ->
        BER_func -> display_pic.m; T3/Main_model_Task_3.m:26-32, :160-185).  payload_bits / payload_packed: as in tx_frames_fused.
        With F = ceil(n_bits / frame_bits), for every SNR of `SNRs` and every repeat r the frames i = 0 .. F - 1 of
        tx_frames_fused(payload, h or fading, SNR, seeds[p], Register, Time_Delay, Freq_Shift) on Philox stream frame0 + r F + i,
        decoded as the matching sweep decodes them -- receiver="task5": rx_chain_task5 as in ber_sweep (the plan's route, its
        MMSE / mmse-ls / OMP-route modes; no Time_Delay / Freq_Shift, time_desync = freq_desync = 0, mp_desync = 1);
        receiver="task4": rx_chain_task4(time_desync, freq_desync, mp_desync) as in ber_sweep_task4.  The refusals of those sweeps
        apply, under the name transport; with Register the plan must descramble with the same register.
        Returns dict(n_bits, frames=F, errors=[n_points, repeats] wrong bits among the payload's n_bits (the zero padding of the
        last frame is sent but not counted), BER = errors / n_bits (BER_func(input_bits, dsc_bits)), loopback = errors == 0 (the
        reference's "Проверка пройдена")
        (+ decoded=[n_points, repeats, ceil(n_bits / 8)] uint8, the received stream joined across frames and cut at n_bits, the
        spare bits of the last byte 0, and decoded_bits=[n_points, repeats, n_bits] 0 / 1, with want_decoded)
        (+ frame_errors=[n_points, repeats, F], per frame over its share of n_bits, with want_frames)
        (+ ones=[n_points, n_bits], the sum over the repeats of decoded bit i -- ones / repeats is the mean received picture, and
        with the payload the per-bit error counts follow -- with want_ones)); torch tensors on `device` (no host synchronisation)
        when it is given, numpy arrays otherwise.  No output depends on max_frames_per_chunk (> 0: the frames of a chunk of the
        plan-owned workspace; a chunk is whole frames and may cut a repeat)."""
        try:
            rcv = {"task5": 5, "task4": 4, 5: 5, 4: 4}[receiver]
        except (KeyError, TypeError):
            raise OfdmError('transport: receiver must be "task5" or "task4"') from None
        keep, n, chan, imp, pr, pts = self._study_args("transport", SNRs, seeds, seed, h, fading, Register, Time_Delay, Freq_Shift)
        pbuf, pp, n_bits = self._payload(device, payload_bits, payload_packed, "transport")
        R = int(repeats)
        F = -(-n_bits // self.frame_bits) if self.frame_bits > 0 else 0
        nb8, Ra = (n_bits + 7) // 8, max(R, 0)                     # (a bad count is the library's refusal)
        (dec, err, fe, ones), ptrs, flags = self._outputs(
            device, ((n, Ra, nb8), np.uint8) if want_decoded else None, ((n, Ra), np.uint64),
            ((n, Ra, F), np.uint32) if want_frames else None, ((n, n_bits), np.uint32) if want_ones else None)
        L.check(self.lib.ofdm_payload_transport(self.handle, rcv, pp, n_bits, R, *chan, *imp, int(time_desync), int(freq_desync),
                                                int(mp_desync), *pts, int(frame0), pr, int(max_frames_per_chunk), *ptrs, flags),
                "transport")
        if device is None:
            err = err.astype(np.int64)
            ber = err / np.float64(max(n_bits, 1))
        else:
            ber = err.double() / torch.full((1,), float(max(n_bits, 1)), dtype=torch.float64, device=err.device)
        out = dict(n_bits=n_bits, frames=F, errors=err, BER=ber, loopback=err == 0)
        if want_decoded:
            out["decoded"] = dec
            if device is None:
                out["decoded_bits"] = np.unpackbits(dec, axis=2)[:, :, :n_bits]
            else:
                sh = torch.arange(7, -1, -1, dtype=torch.int16, device=dec.device)
                out["decoded_bits"] = ((dec.to(torch.int16).unsqueeze(-1) >> sh) & 1).to(torch.uint8).reshape(n, Ra, -1)[:, :, :n_bits]
        if want_frames:
            out["frame_errors"] = fe
        if want_ones:
            out["ones"] = ones
        return out

    def estimator_study(self, SNRs, frames_per_point, h=None, fading=None, mmse="ls", seeds=None, seed=1, frame0=0, device=None,
                        want_frames=False, max_frames_per_chunk=0):
        """The estimator comparison of Task 5 in one device-resident call (ofdm_estimator_study): LS_CE, MMSE_CE, MP_estimate and
        OMP_estimate on the same received frame of every channel realisation (T5/Task5_part2.m:148-205, :269-304; over SNR
        T5/Main_model_Task_5.m:303-346).  For every SNR of `SNRs` the frames frame0 .. frame0 + frames_per_point - 1 of
        tx_frames_fused(h or fading, SNR, seeds[p]), bit for bit, through the estimator stages of task5_part2_tile, each estimate
        equalised and demapped against the frame's own payload.  The plan's receiver modes (MMSE, mmse-ls, OMP route) are not read;
        a plan with a DeScrambler is refused.  mmse="ls": MMSE_CE with h = ifft(H_LS) of the frame at the point's SNR
        (Main_model_Task_5.m:314-315); mmse="genie": with the frame's true taps (Task5_part2.m:176-177), a frame with no tap below
        N_carrier counted in nmse_dropped.
        Returns dict(rows=("LS", "MMSE", "MP", "OMP"), the order of every trailing 4; errors=[n_points, 4] int64 bit errors,
        bits=bits counted per point and row, BER = errors / bits; nmse_sums=[n_points, 4] float64, per point the sum over its
        frames, in frame order, of sum_k |fft(h_f, Nfft)(k) - H_e,f(k)|^2 on carriers 1..N_carrier, a frame whose sum is not
        finite left out and counted in nmse_dropped=[n_points, 4] int64; NMSE = nmse_sums / ((frames_per_point - nmse_dropped)
        * N_carrier), the normalisation of ber_sweep(want_nmse=True) with the dropped frames taken out (+ frame_errors=[n_points,
        frames_per_point, 4] int64 / uint32, frame_nmse=[n_points, frames_per_point, 4] float64 with want_frames)); torch tensors
        on `device` (no host synchronisation) when it is given, numpy arrays otherwise.  No output depends on
        max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned workspace)."""
        try:
            mode = {"ls": 0, "genie": 1}[mmse]
        except (KeyError, TypeError):
            raise OfdmError('estimator_study: mmse must be "ls" or "genie"') from None
        keep, n, chan, _, _, pts = self._study_args("estimator_study", SNRs, seeds, seed, h, fading, None, None, None)
        fpp = int(frames_per_point)
        fa = max(fpp, 0)
        (err, ns, drop, fe, fn), ptrs, flags = self._outputs(
            device, ((n, 4), np.uint64), ((n, 4), np.float64), ((n, 4), np.uint64), ((n, fa, 4), np.uint32) if want_frames else None,
            ((n, fa, 4), np.float64) if want_frames else None)
        L.check(self.lib.ofdm_estimator_study(self.handle, *chan, *pts, fpp, int(frame0), mode, int(max_frames_per_chunk), *ptrs,
                                              flags), "estimator_study")
        (err, drop), _, f64 = self._counts(device, None, err, drop)
        bits = fa * self.frame_bits
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame counted: NaN, the mean of nothing
            ber = f64(err) / float(bits) if bits else f64(err) * float("nan")
            nmse = ns / (f64(fpp - drop) * float(self.N_carrier))
        out = dict(rows=("LS", "MMSE", "MP", "OMP"), errors=err, bits=bits, BER=ber, nmse_sums=ns, nmse_dropped=drop, NMSE=nmse)
        if want_frames:
            out.update(frame_errors=fe, frame_nmse=fn)
        return out

    def estimator_profile(self, SNRs, frames_per_point, h=None, fading=None, mmse="ls", bins=dict(n=60, lo=-50.0, hi=10.0), seeds=None,
                          seed=1, frame0=0, device=None, want_frames=False, max_frames_per_chunk=0):
        """estimator_study with its two pictures, in one device-resident call (ofdm_estimator_profile): per point the curves
        |H_freq| against |H_est_LS|, |H_est_MMSE|, |H_est_MP|, |H_est_OMP| over the carriers (T5/Main_model_Task_5.m:207-231) and
        |H_tau| against the delays OMP_estimate picked (:238-242), summed over the point's frames, with the histogram of the
        frames' error.  The arguments of estimator_study plus bins = dict(n, lo, hi), the histogram of the frames by
        10 log10(frame_nmse / N_carrier) in dB; the same frames, the same refusals under the name estimator_profile.
        Returns everything estimator_study returns for the same arguments, bit for bit (rows, errors, bits, BER, nmse_sums,
        nmse_dropped, NMSE (+ frame_errors, frame_nmse with want_frames)), and, with nc = N_carrier, K = the plan's dictionary
        columns, T = dominant_taps:
        true_amp_sums=[n_points, nc] float64 = sum_f |H_f(k)| over all frames; est_amp_sums, err_sums, amp_err_sums=[n_points, 4,
        nc] = sum_f |H_e,f(k)|, sum_f |H_f(k) - H_e,f(k)|^2, sum_f (|H_e,f(k)| - |H_f(k)|)^2 in frame order, a frame whose
        frame_nmse[e] is not finite left out (the rule and the count of nmse_dropped); mean_true_amp = true_amp_sums /
        frames_per_point, mean_est_amp = est_amp_sums / (frames_per_point - nmse_dropped), nmse_profile = err_sums /
        (frames_per_point - nmse_dropped);
        nmse_hist=[n_points, 4, bins.n], nmse_below, nmse_above, nmse_nan=[n_points, 4] int64 (their sum is frames_per_point;
        nmse_nan = nmse_dropped), edges=[bins.n + 1] in dB and thresholds=[bins.n + 1] = N_carrier 10^(edges / 10), the table the
        frames were compared against (numpy, made on the host);
        for OMP_estimate: pick_hist=[n_points, K] int64, the pick slots whose 0-based delay is k; tap_amp_sums=[n_points, K]
        float64 = sum |x| of those slots (sum_f |est_fade_chan_f(k)|); n_picks_hist=[n_points, T + 1] int64, the frames by the
        number of picks made; true_tap_amp_sums=[n_points, K] = sum_f |a_f,t| at each channel tap's delay d_t < K;
        true_outside=[n_points] int64, the channel taps with d_t >= K counted per frame; support_hits, support_misses,
        support_false=[n_points] int64: the delays in both the frame's true support (d_t < K) and its distinct picks, in the
        true support only, in the picks only (+ picks=[n_points, frames_per_point, T] int32, 1-based, 0 = not made, and
        tap_x=[n_points, frames_per_point, T] complex128 with want_frames).  MP_estimate's delay-domain curve is not offered: the
        tap workspace holds one pursuit at a time; its per-carrier rows are there.
        torch tensors on `device` (no host synchronisation) when it is given, numpy arrays otherwise.  No output depends on
        max_frames_per_chunk (> 0: the frames of a chunk of the plan-owned workspace)."""
        try:
            mode = {"ls": 0, "genie": 1}[mmse]
        except (KeyError, TypeError):
            raise OfdmError('estimator_profile: mmse must be "ls" or "genie"') from None
        try:
            extra = set(bins) - {"n", "lo", "hi"}
            bn, blo, bhi = int(bins["n"]), float(bins["lo"]), float(bins["hi"])
        except (TypeError, KeyError, ValueError):
            raise OfdmError("estimator_profile: bins must be dict(n=, lo=, hi=)") from None
        if extra:
            raise OfdmError(f"estimator_profile: unknown bins keys {sorted(extra)}")
        keep, n, chan, _, _, pts = self._study_args("estimator_profile", SNRs, seeds, seed, h, fading, None, None, None)
        fpp = int(frames_per_point)
        fa, nb = max(fpp, 0), bn if 1 <= bn <= 4096 else 0       # (a bad count is the library's refusal)
        nc, K, T = self.N_carrier, self.K, self.taps
        fr = lambda shape, dt: (shape, dt) if want_frames else None
        (err, ns, drop, fe, fn, tsum, esum, esq, aerr, hist, below, above, hnan, pick, tamp, npk, ttamp, outside, supp, picks, tx), \
            ptrs, flags = self._outputs(
                device, ((n, 4), np.uint64), ((n, 4), np.float64), ((n, 4), np.uint64), fr((n, fa, 4), np.uint32),
                fr((n, fa, 4), np.float64), ((n, nc), np.float64), ((n, 4, nc), np.float64), ((n, 4, nc), np.float64),
                ((n, 4, nc), np.float64), ((n, 4, nb), np.uint64), ((n, 4), np.uint64), ((n, 4), np.uint64), ((n, 4), np.uint64),
                ((n, K), np.uint64), ((n, K), np.float64), ((n, T + 1), np.uint64), ((n, K), np.float64), ((n,), np.uint64),
                ((n, 3), np.uint64), fr((n, fa, T), np.int32), fr((n, fa, T), np.complex128))
        thr = np.zeros(nb + 1, np.float64)
        L.check(self.lib.ofdm_estimator_profile(self.handle, *chan, *pts, fpp, int(frame0), mode, int(max_frames_per_chunk), bn, blo,
                                                bhi, *ptrs[:13], thr.ctypes.data_as(C.c_void_p), *ptrs[13:], flags),
                "estimator_profile")
        (err, drop, hist, below, above, hnan, pick, npk, outside, supp), count, f64 = self._counts(
            device, fpp, err, drop, hist, below, above, hnan, pick, npk, outside, supp)
        bits = fa * self.frame_bits
        with np.errstate(divide="ignore", invalid="ignore"):     # no frame counted: NaN, the mean of nothing
            ber = f64(err) / float(bits) if bits else f64(err) * float("nan")
            nmse = ns / (f64(fpp - drop) * float(nc))
            kept = f64(fpp - drop)[..., None]
            mean_true, mean_est, profile = tsum / count, esum / kept, esq / kept
        out = dict(rows=("LS", "MMSE", "MP", "OMP"), errors=err, bits=bits, BER=ber, nmse_sums=ns, nmse_dropped=drop, NMSE=nmse,
                   true_amp_sums=tsum, est_amp_sums=esum, err_sums=esq, amp_err_sums=aerr, mean_true_amp=mean_true,
                   mean_est_amp=mean_est, nmse_profile=profile, nmse_hist=hist, nmse_below=below, nmse_above=above, nmse_nan=hnan,
                   edges=np.linspace(blo, bhi, nb + 1), thresholds=thr, pick_hist=pick, tap_amp_sums=tamp, n_picks_hist=npk,
                   true_tap_amp_sums=ttamp, true_outside=outside, support_hits=supp[:, 0], support_misses=supp[:, 1],
                   support_false=supp[:, 2])
        if want_frames:
            out.update(frame_errors=fe, frame_nmse=fn, picks=picks, tap_x=tx)
        return out

    def ber_sweep(self, SNRs, frames_per_point, h=None, seeds=None, seed=1, frame0=0, Register=None, device=None,
                  want_frame_errors=False, max_frames_per_chunk=0, want_mer=False, want_frame_mer=False, fading=None,
                  want_nmse=False, want_frame_nmse=False, density=None):
        """One device-resident tile of a BER(SNR) sweep (ofdm_ber_sweep_task5): for every SNR of `SNRs` the frames
        frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h, SNR, seeds[p]) decoded by rx_chain_task5 on this plan
        (T3/Main_model_Task_3.m:237-268, T5/Task5_part2.m:134,:148-152).  seeds: one Philox key per point (default: `seed`
        for every point).  With Register the plan must descramble with the same register (set_descrambler) and the
        errors count against the payload bits.
        Returns dict(errors=[n_points] int64 bit errors, bits=bits counted per point, frame_errors=[n_points,
        frames_per_point] (with want_frame_errors)); torch tensors on `device` (no host synchronisation) when it is given,
        numpy arrays otherwise.
        want_mer (ofdm_ber_sweep_task5_ex): also mer_sums=[n, 2], the MER_func sums of each point's frames (the whole RX_IQ,
        frames concatenated; T5/Main_model_Task_5.m:282), and MER_dB=[n] (computed on `device` when it is given); with
        want_frame_mer the per-frame sums frame_mer_sums=[n, frames_per_point, 2].
        fading=(delays, powers) (ofdm_ber_sweep_task5_fading; not with h): the frames of tx_frames_fused(fading=...), a channel
        realisation per frame (T5/Task5_part2.m:148-155).  want_nmse then adds nmse_sums=[n], per point the sum over its frames
        of sum_k |fft(h_f, Nfft)(k) - H_est_f(k)|^2 on carriers 1..N_carrier, and NMSE=[n] = nmse_sums / (frames_per_point *
        N_carrier) (T5/Task5_part2.m:202-205,:318); want_frame_nmse the per-frame sums frame_nmse=[n, frames_per_point].
        density=dict(bins=, half_width=, skip=0) (ofdm_ber_sweep_task5_scope; with h or with fading): also density=[n, bins,
        bins] int64, per point the count of its frames' equalised points RX_IQ (those of rx_chain_task5(iq_window=), from
        0-based index skip on) at [row of im, column of re] with col = clamp(floor((re + half_width) * bins / (2 half_width)),
        0, bins - 1), and density_dropped=[n], the points with a non-finite coordinate, which are not binned: sum(density[p])
        + density_dropped[p] = frames_per_point * (nd * N_symb - skip).  The scatter of T5/Main_model_Task_5.m:248-251 at sweep
        sizes, over the points MER_func sums at :282."""
        if want_frame_mer and not want_mer:
            raise OfdmError("ber_sweep: want_frame_mer needs want_mer")
        if (want_nmse or want_frame_nmse) and fading is None:
            raise OfdmError("ber_sweep: want_nmse / want_frame_nmse need fading")
        if density is not None:
            bins, half_width, skip = self._density_args(density, "ber_sweep")
        snr, sd, psnr, psd = self._points(SNRs, seeds, seed, "ber_sweep")
        n, fpp = snr.size, int(frames_per_point)
        (err, fe, ms, fm, ns, fn), ptrs, flags = self._outputs(
            device, ((n,), np.uint64), ((n, fpp), np.uint32) if want_frame_errors else None,
            ((n, 2), np.float64) if want_mer else None, ((n, fpp, 2), np.float64) if want_frame_mer else None,
            ((n,), np.float64) if want_nmse else None, ((n, fpp), np.float64) if want_frame_nmse else None)
        own = {}
        if density is not None:
            dptrs, own = self._density_outputs(device, n, bins)
        keep, chan, taps, pr = self._sweep_channel(h, fading, Register, "ber_sweep")
        pts = (psnr, psd, n, fpp, int(frame0), pr, int(max_frames_per_chunk))
        if density is not None:
            L.check(self.lib.ofdm_ber_sweep_task5_scope(self.handle, *taps, *pts, *ptrs, *chan, *dptrs, bins, half_width, skip,
                                                        flags), "ber_sweep_task5_scope")
        elif fading is not None:
            L.check(self.lib.ofdm_ber_sweep_task5_fading(self.handle, *taps, *pts, *ptrs, flags), "ber_sweep_task5_fading")
        else:
            L.check(self.lib.ofdm_ber_sweep_task5_ex(self.handle, *chan, *pts, *ptrs[:4], flags),
                    "ber_sweep_task5_ex" if want_mer else "ber_sweep_task5")
        return self._sweep_result(device, err, fpp, own, ns, fn, fe, ms, fm)

    def _sweep_result(self, device, errors, fpp, own, nmse_sums, frame_nmse, frame_errors, mer_sums, frame_mer_sums):
        """What ber_sweep and ber_sweep_task4 return alike: the errors (int64 on the host), the bits per point, `own` (what only
        one of them has), then each output that was wanted (None: not wanted) with the figures derived from it."""
        out = dict(errors=errors if device is not None else errors.astype(np.int64), bits=fpp * self.frame_bits, **own)
        if nmse_sums is not None:
            out["nmse_sums"] = nmse_sums
            out["NMSE"] = nmse_sums / float(max(fpp, 1) * self.N_carrier)
        if frame_nmse is not None:
            out["frame_nmse"] = frame_nmse
        if frame_errors is not None:
            out["frame_errors"] = frame_errors
        if mer_sums is not None:
            out["mer_sums"] = mer_sums
            out["MER_dB"] = _mer_db(mer_sums)
            if frame_mer_sums is not None:
                out["frame_mer_sums"] = frame_mer_sums
        return out

    def ber_sweep_task4(self, SNRs, frames_per_point, h=None, Time_Delay=None, Freq_Shift=None, time_desync=None,
                        freq_desync=None, mp_desync=None, seeds=None, seed=1, frame0=0, Register=None, device=None,
                        want_frame_errors=False, max_frames_per_chunk=0, want_mer=False, mer_skip=0,
                        want_frame_mer=False, fading=None, want_nmse=False, want_frame_nmse=False, density=None):
        """One device-resident tile of a BER(SNR) sweep of the Task-4 receiver (ofdm_ber_sweep_task4): for every SNR of
        `SNRs` the frames frame0 .. frame0 + frames_per_point - 1 of tx_frames_fused(h, SNR, seeds[p], Time_Delay,
        Freq_Shift) decoded by rx_chain_task4(time_desync, freq_desync, mp_desync) on this plan.  A desync flag left at None
        follows its impairment, as the single flag of T4/Main_model_Task_4.m:81-110 switches both: time_desync = Time_Delay
        given, freq_desync = Freq_Shift given, mp_desync = h given.  All flags off, no STO / CFO / h: the BER(SNR) loop of
        T3/Main_model_Task_3.m:237-268.  Register: as in ber_sweep (the plan must descramble with the same register).
        Returns dict(errors=[n] bit errors, bits=bits counted per point, status_counts=[n, 4] frames with rx_chain_task4
        status 0, 1, -1, -2, cfo_abs_err=[n] sum of |FreqOffset + IFO - Freq_Shift| over the point's frames (0 with
        freq_desync off) (+ frame_errors=[n, frames_per_point] with want_frame_errors)); torch tensors on `device` (no host
        synchronisation) when it is given, numpy arrays otherwise.
        want_mer (ofdm_ber_sweep_task4_ex): also mer_sums=[n, 2], the MER_func sums of each point's frames (RX_IQ from
        0-based index mer_skip on, frames concatenated), and MER_dB=[n] (computed on `device` when it is given); with
        want_frame_mer the per-frame sums frame_mer_sums=[n, frames_per_point, 2].  Time_Delay=12, time_desync=1,
        freq_desync=0, mp_desync=0, mer_skip=Nfft+T_guard is the MER(SNR) study of T4/Main_model_Task_4.m:136-200.
        fading=(delays, powers) (ofdm_ber_sweep_task4_fading; not with h): the frames of tx_frames_fused(fading=..., Time_Delay,
        Freq_Shift), a channel realisation per frame (T5/Task5_part2.m:148-155); mp_desync left at None is then on.
        want_nmse (ofdm_ber_sweep_task4_nmse / _fading; needs mp_desync): also nmse_sums=[n], per point the sum over its frames
        of sum_k |H(k) - H_est_f(k)|^2 on carriers 1..N_carrier against fft(h, Nfft), or with fading against the frame's own
        channel, and NMSE=[n] = nmse_sums / (frames_per_point * N_carrier) (T4/Main_model_Task_4.m:205-239); with
        want_frame_nmse the per-frame sums frame_nmse=[n, frames_per_point].  The plain difference of the reference: with
        time_desync / freq_desync on, fine_sync has taken the channel's mean delay and common phase out of what
        estimate_channel sees, and the difference contains that ramp.
        density=dict(bins=, half_width=, skip=0) (ofdm_ber_sweep_task4_scope; not with fading): also density=[n, bins, bins]
        int64, per point the count of its frames' equalised points RX_IQ (those of rx_chain_task4(iq_window=), from 0-based
        index skip on) at [row of im, column of re] with col = clamp(floor((re + half_width) * bins / (2 half_width)), 0,
        bins - 1), and density_dropped=[n], the points with a non-finite coordinate, which are not binned: sum(density[p]) +
        density_dropped[p] = frames_per_point * (nd * N_symb - skip).  The constellation per SNR point of
        T4/Main_model_Task_4.m:137-203 (:165) at sweep sizes."""
        if want_frame_nmse and not want_nmse:
            raise OfdmError("ber_sweep_task4: want_frame_nmse needs want_nmse")
        if density is not None:
            if fading is not None:
                raise OfdmError("ber_sweep_task4: density is not available with fading")
            bins, half_width, skip = self._density_args(density, "ber_sweep_task4")
        snr, sd, psnr, psd = self._points(SNRs, seeds, seed, "ber_sweep_task4")
        n, fpp = snr.size, int(frames_per_point)
        sm, sv = _imp_mode(Time_Delay, "ber_sweep_task4")
        cm, cv = _imp_mode(Freq_Shift, "ber_sweep_task4")
        td = Time_Delay is not None if time_desync is None else bool(time_desync)
        fd = Freq_Shift is not None if freq_desync is None else bool(freq_desync)
        md = (h is not None or fading is not None) if mp_desync is None else bool(mp_desync)
        (err, stc, cae, fe, ms, fm, ns, fn), ptrs, flags = self._outputs(
            device, ((n,), np.uint64), ((n, 4), np.uint64), ((n,), np.float64),
            ((n, fpp), np.uint32) if want_frame_errors else None, ((n, 2), np.float64) if want_mer else None,
            ((n, fpp, 2), np.float64) if want_mer and want_frame_mer else None, ((n,), np.float64) if want_nmse else None,
            ((n, fpp), np.float64) if want_frame_nmse else None)
        grids = {}
        if density is not None:
            dptrs, grids = self._density_outputs(device, n, bins)
        keep, chan, taps, pr = self._sweep_channel(h, fading, Register, "ber_sweep_task4")
        # what every entry takes behind its channel: up to frame_mer_sums_out, the arguments of ofdm_ber_sweep_task4_ex
        head = (self.handle, *(chan if fading is None else taps), sm, int(sv), cm, float(cv), int(td), int(fd), int(md), psnr, psd,
                n, fpp, int(frame0), pr, int(max_frames_per_chunk), *ptrs[:4], int(mer_skip) if want_mer else 0, *ptrs[4:6])
        if density is not None:
            L.check(self.lib.ofdm_ber_sweep_task4_scope(*head, *ptrs[6:], *dptrs, bins, half_width, skip, flags),
                    "ber_sweep_task4_scope")
        elif fading is not None:
            L.check(self.lib.ofdm_ber_sweep_task4_fading(*head, *ptrs[6:], flags), "ber_sweep_task4_fading")
        elif want_nmse:
            L.check(self.lib.ofdm_ber_sweep_task4_nmse(*head, *ptrs[6:], flags), "ber_sweep_task4_nmse")
        else:
            L.check(self.lib.ofdm_ber_sweep_task4_ex(*head, flags), "ber_sweep_task4_ex" if want_mer else "ber_sweep_task4")
        own = dict(status_counts=stc.astype(np.int64) if device is None else stc, cfo_abs_err=cae, **grids)
        return self._sweep_result(device, err, fpp, own, ns, fn, fe, ms, fm)

    def set_timing(self, enable=True):
        L.check(self.lib.ofdm_rx_plan_set_timing(self.handle, int(bool(enable))), "rx_plan_set_timing")

    def last_kernel_ms(self):
        """(symbol-1 kernel, OMP kernel, symbols kernel) milliseconds of the last chain call (HIP events)."""
        ms = (C.c_float * 3)()
        L.check(self.lib.ofdm_rx_plan_last_kernel_ms(self.handle, ms), "rx_plan_last_kernel_ms")
        return tuple(float(v) for v in ms)

    def last_stage_ms(self):
        """Stage milliseconds of the last rx_chain_task4 call (HIP events on the launch stream)."""
        ms = (C.c_float * 5)()
        L.check(self.lib.ofdm_rx_plan_last_task4_ms(self.handle, ms), "rx_plan_last_task4_ms")
        return dict(zip(("AutoCorrFunction", "remove_IFO", "OFDM_demodulator", "fine_sync+estimate_channel", "equalize+demap"),
                        (float(v) for v in ms)))

    def close(self):
        if getattr(self, "handle", None):
            self.lib.ofdm_rx_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def rx_chain_task5(plan: RxPlan, rx, ref_bits_packed=None, want_h=False, want_index=False, want_mer=False, iq_window=None):
    """Fused demod -> OMP -> equalise -> payload -> demap -> BER over a batch of frames.

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).
    Returns dict(bits=[n_frames, frame_bytes] uint8 packed MSB-first (frame-major), errors=[n_frames] uint32 or None,
    H=[N_carrier, n_frames] or None, index=[taps, n_frames] int32 or None).
    want_mer (ofdm_rx_chain_task5_ex): also mer_sums=[n_frames, 2] float64, the sums {|ideal|^2, |ideal - RX_IQ|^2} of
    MER_func (T5/MER_func.m:3-25) over each frame's whole RX_IQ (T5/Main_model_Task_5.m:282), and MER_dB=[n_frames] =
    10 log10(s1 / s2).
    iq_window=(first, count) (ofdm_rx_chain_task5_iq): also RX_IQ=[n_frames, count] complex in the plan's precision, the
    equalised points get_payload(.)(:) of each frame from 0-based index first on -- what the demapper slices and MER_func sums;
    (nd, 332) is the scatterplot(RX_IQ(nd+1 : nd+332)) of T5/Main_model_Task_5.m:248-251.  The other outputs are those of the
    call with want_mer."""
    call, nfr, iq, bits, errors, pbits = _rx_chain_front("rx_chain_task5", plan, rx, ref_bits_packed, iq_window)
    H, pH = (call.cout((plan.N_carrier, nfr)) if want_h else (None, None))
    idx, pidx = (call._out((plan.taps, nfr), np.int32, torch.int32 if call.dev else None) if want_index else (None, None))
    return _rx_chain_tail("rx_chain_task5", plan, call, rx, nfr, dict(bits=bits, errors=errors, H=H, index=idx),
                          (*pbits, pH, pidx), want_mer, iq)


def _rx_chain_front(what, plan, rx, ref_bits_packed, iq_window):
    """What rx_chain_task4 and rx_chain_task5 (`what`) do alike before their own outputs: the row check, iq_window as (first,
    count) or None, the packed bits [n_frames, frame_bytes] and, with reference bits, the errors [n_frames] -> (call, n_frames,
    iq_window, bits, errors, the pointers (bits_out, ref_bits, errors_out))."""
    call = _Call(rx, f64=plan.f64)
    rows, nfr = _shape2(rx)
    if rows != plan.frame_samples:
        raise OfdmError(f"{what}: rx must have (Nfft+T_guard)*N_symb rows")
    iq = None
    if iq_window is not None:
        try:
            iq_first, iq_count = (int(v) for v in iq_window)
        except (TypeError, ValueError):
            raise OfdmError(f"{what}: iq_window must be (first, count)") from None
        iq = (iq_first, iq_count)
    flat_bits, pbits = call._out((plan.frame_bytes * nfr,), np.uint8, torch.uint8 if call.dev else None)
    bits = flat_bits.reshape(nfr, plan.frame_bytes)
    pref, errors, perr = None, None, None
    if ref_bits_packed is not None:
        ref = ref_bits_packed
        if tuple(ref.shape) != (nfr, plan.frame_bytes):
            raise OfdmError(f"{what}: ref_bits_packed must be [n_frames, frame_bytes]")
        ref = ref.contiguous().view(-1) if _is_torch(ref) else np.ascontiguousarray(ref).reshape(-1)
        pref = call._flat(ref, np.uint8, torch.uint8 if call.dev else None)[0]
        errors, perr = call._out((nfr,), np.uint32, torch.int32 if call.dev else None)
    return call, nfr, iq, bits, errors, (pbits, pref, perr)


def _rx_chain_tail(what, plan, call, rx, nfr, out, args, want_mer, iq, mer_args=()):
    """The call itself and what it adds to `out`: ofdm_<what> without the MER sums and the window, else ofdm_<what>_ex or, with
    the window iq = (first, count), ofdm_<what>_iq.  args: the receiver's own arguments and output pointers, as all three
    entries take them behind n_frames; mer_args: what _ex and _iq take between those and mer_sums_out."""
    if not want_mer and iq is None:
        L.check(getattr(call.lib, f"ofdm_{what}")(plan.handle, call.cin(rx), nfr, *args, call.flags), what)
        return out
    mer, pmer = None, None
    if want_mer:
        mer, pmer = call._out((2, nfr), np.float64, torch.float64 if call.dev else None)     # memory [n_frames][2]
        mer = mer.T
        out.update(mer_sums=mer)
    head = (plan.handle, call.cin(rx), nfr, *args, *mer_args, pmer)
    if iq is None:
        L.check(getattr(call.lib, f"ofdm_{what}_ex")(*head, call.flags), f"{what}_ex")
    else:
        buf, piq = call.cout((max(iq[1], 0), nfr))                                        # memory [n_frames][count]
        L.check(getattr(call.lib, f"ofdm_{what}_iq")(*head, *iq, piq, call.flags), f"{what}_iq")
        out.update(RX_IQ=buf.T)
    if want_mer:
        out.update(MER_dB=_mer_db(mer))
    return out


def rx_chain_task4(plan: RxPlan, rx, time_desync=1, freq_desync=1, mp_desync=1, ref_bits_packed=None, want_h=False,
                   want_mer=False, mer_skip=0, iq_window=None):
    """Task-4 receiver over a batch of frames (T4/Main_model_Task_4.m:278-347 per frame): AutoCorrFunction -> add_STO x2 ->
    add_CFO -> remove_IFO -> OFDM_demodulator -> fine_sync -> estimate_channel -> equalize_signal -> get_payload -> demapping.

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).
    Returns dict(bits=[n_frames, frame_bytes] packed demapped bits (not descrambled), errors vs ref_bits_packed or None,
    TgPosition=[n_frames] int64, FreqOffset=[n_frames] float64, IFO=[n_frames] int32, status=[n_frames] int32
    (0 ok, 1 AutoCorrFunction fallback, -1 no IFO line, -2 TgPosition out of range), H=[N_carrier, n_frames] or None).
    want_mer (ofdm_rx_chain_task4_ex): also mer_sums=[n_frames, 2] float64, the sums {|ideal|^2, |ideal - RX_IQ|^2} of
    MER_func (T5/MER_func.m:3-25) over each frame's get_payload(.)(:) from 0-based index mer_skip on (Nfft + T_guard =
    RX_IQ(Nfft+T_Guard+1:end) of T4/Main_model_Task_4.m:163), and MER_dB=[n_frames] = 10 log10(s1 / s2).
    iq_window=(first, count) (ofdm_rx_chain_task4_iq): also RX_IQ=[n_frames, count] complex in the plan's precision, the
    equalised points get_payload(.)(:) of each frame from 0-based index first on -- what the demapper slices and MER_func sums;
    (nd, nd) is the scatterplot(RX_IQ(length(dataCarriers)+1 : 2*length(dataCarriers))) of T4/Main_model_Task_4.m:165."""
    call, nfr, iq, bits, errors, pbits = _rx_chain_front("rx_chain_task4", plan, rx, ref_bits_packed, iq_window)
    tg, ptg = call._out((nfr,), np.int64, torch.int64 if call.dev else None)
    fo, pfo = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    ifo, pifo = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    stt, pst = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    H, pH = (call.cout((plan.N_carrier, nfr)) if want_h else (None, None))
    return _rx_chain_tail("rx_chain_task4", plan, call, rx, nfr,
                          dict(bits=bits, errors=errors, TgPosition=tg, FreqOffset=fo, IFO=ifo, status=stt, H=H),
                          (int(bool(time_desync)), int(bool(freq_desync)), int(bool(mp_desync)), *pbits, ptg, pfo, pifo, pst, pH),
                          want_mer, iq, mer_args=(int(mer_skip) if want_mer else 0,))


def rx_spectrum(plan: RxPlan, rx, first=None, n_windows=1, want_power=False):
    """The amplitude spectrum of received frames (ofdm_rx_spectrum): abs(fft(Rx_OFDM_Signal(T_Guard+1 : Nfft+T_Guard))) of
    T3/Main_model_Task_3.m:138 and T5/Main_model_Task_5.m:131 with the defaults; first = T_guard + (Nfft + T_guard) is the useful
    part of symbol 2 (T4/Main_model_Task_4.m:268).

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).  Window w = 0 .. n_windows - 1
    of a frame is its samples first + w (Nfft + T_guard) .. + Nfft - 1 (0-based; first defaults to T_guard); it may start anywhere
    and straddle a symbol boundary, and must end inside the frame.
    Returns dict(amp=[n_frames, n_windows, Nfft] real in the plan's precision, |fft(window)| (forward, unscaled), power =
    [n_frames, Nfft] float64 with want_power, per bin the sum over the windows of re^2 + im^2 in double, else None)."""
    call = _Call(rx, f64=plan.f64)
    rows, nfr = _shape2(rx)
    if rows != plan.frame_samples:
        raise OfdmError("rx_spectrum: rx must have (Nfft+T_guard)*N_symb rows")
    first = plan.T_guard if first is None else int(first)
    nw = int(n_windows)
    rdt = np.float64 if plan.f64 else np.float32
    n_alloc = nw if 0 <= nw <= plan.N_symb else 0                 # (a count that cannot fit is the library's refusal)
    amp, pamp = call._out((nfr * n_alloc * plan.Nfft,), rdt, _torch_dtype(rdt) if call.dev else None)
    power, ppow = (call._out((nfr * plan.Nfft,), np.float64, torch.float64 if call.dev else None) if want_power else (None, None))
    L.check(call.lib.ofdm_rx_spectrum(plan.handle, call.cin(rx), nfr, first, nw, pamp, ppow, call.flags), "rx_spectrum")
    return dict(amp=amp.reshape(nfr, n_alloc, plan.Nfft), power=None if power is None else power.reshape(nfr, plan.Nfft))


def rx_acf(plan: RxPlan, rx, width=None, want_rho=False):
    """The coarse synchroniser's curve of received frames (ofdm_rx_acf): abs(AutoCorr) of AutoCorrFunction(frame, width, Nfft), the
    plot of T4/Main_model_Task_4.m:282-287, with the function's TgPosition and FreqOffset; width=None is T_guard (T4:278).

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).
    Returns dict(amp=[n_frames, n_out] real in the plan's precision, n_out = frame_samples - width - Nfft, |rho| formed in double
    from rho and rounded; rho=[n_frames, n_out] complex with want_rho, else None: bit for bit the AutoCorr row of AutoCorrFunction
    on that frame (0 / 0 = NaN for a window of zeros); tg_position=[n_frames] int64 (1-based); status=[n_frames] int32 (0 ok, 1 the
    catch branch: TgPosition 65, no warning is issued); freq_offset=[n_frames] float64)."""
    call = _Call(rx, f64=plan.f64)
    rows, nfr = _shape2(rx)
    if rows != plan.frame_samples:
        raise OfdmError("rx_acf: rx must have (Nfft+T_guard)*N_symb rows")
    W = plan.T_guard if width is None else int(width)
    n_out = max(plan.frame_samples - W - plan.Nfft, 0) if 1 <= W <= 1024 else 0          # (a bad width is the library's refusal)
    rdt = np.float64 if plan.f64 else np.float32
    amp, pamp = call._out((nfr * n_out,), rdt, _torch_dtype(rdt) if call.dev else None)
    rho, prho = (call.cout((nfr * n_out,)) if want_rho else (None, None))
    tg, ptg = call._out((nfr,), np.int64, torch.int64 if call.dev else None)
    stt, pst = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    fo, pfo = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    L.check(call.lib.ofdm_rx_acf(plan.handle, call.cin(rx), nfr, W, pamp, prho, ptg, pst, pfo, call.flags), "rx_acf")
    return dict(amp=amp.reshape(nfr, n_out), rho=None if rho is None else rho.reshape(nfr, n_out), tg_position=tg, status=stt,
                freq_offset=fo)


_IFO_STAGES = {"raw": 0, "receiver": 1}


def _ifo_stage(stage, what):
    """"raw" / "receiver" -> the library's 0 / 1; a number goes through as it is (the library refuses what is neither)."""
    if isinstance(stage, str):
        if stage not in _IFO_STAGES:
            raise OfdmError(f"{what}: stage must be 'raw' or 'receiver'")
        return _IFO_STAGES[stage]
    return int(stage)


def rx_ifo(plan: RxPlan, rx, stage="receiver", time_desync=1, want_amp=True):
    """The spectrum remove_IFO thresholds, for received frames (ofdm_rx_ifo): abs(fft(rx_signal(Nfft+1 : 2*Nfft))) of
    T4/remove_IFO.m:5 and IFO = inds(1) - 1 (:6-8).  stage="raw": the frame as it is (T4/Main_model_Task_4.m:124-125);
    stage="receiver": what the Task-4 receiver hands remove_IFO (T4:278-303) -- with time_desync add_STO(rx, TgPosition) and
    add_STO(., -(Nfft + T_guard)), then add_CFO(., -FreqOffset), rounded as the receiver's stages round.  TgPosition and FreqOffset
    are AutoCorrFunction(frame, T_guard, Nfft)'s in both stages, bit for bit those of rx_chain_task4(time_desync, 1, 0).

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).
    Returns dict(amp=[n_frames, Nfft] real in the plan's precision with want_amp, else None: |S| formed in double and rounded;
    ifo=[n_frames] int32, the first bin above 0.77, 0 where there is none; status=[n_frames] int32 (0 ok, 1 AutoCorrFunction's
    catch branch, -1 no bin above 0.77, -2 as in rx_chain_task4); n_above=[n_frames] int32, the bins above 0.77;
    tg_position=[n_frames] int64 (1-based); freq_offset=[n_frames] float64)."""
    call = _Call(rx, f64=plan.f64)
    rows, nfr = _shape2(rx)
    if rows != plan.frame_samples:
        raise OfdmError("rx_ifo: rx must have (Nfft+T_guard)*N_symb rows")
    rdt = np.float64 if plan.f64 else np.float32
    amp, pamp = (call._out((nfr * plan.Nfft,), rdt, _torch_dtype(rdt) if call.dev else None) if want_amp else (None, None))
    ifo, pifo = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    stt, pst = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    na, pna = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    tg, ptg = call._out((nfr,), np.int64, torch.int64 if call.dev else None)
    fo, pfo = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    L.check(call.lib.ofdm_rx_ifo(plan.handle, call.cin(rx), nfr, _ifo_stage(stage, "rx_ifo"), int(time_desync), pamp, pifo, pst, pna, ptg, pfo,
                                 call.flags), "rx_ifo")
    return dict(amp=None if amp is None else amp.reshape(nfr, plan.Nfft), ifo=ifo, status=stt, n_above=na, tg_position=tg,
                freq_offset=fo)


def rx_hest(plan: RxPlan, rx, time_desync=1, freq_desync=1, want_h=True, want_pilots=True):
    """Both outputs of estimate_channel for received frames (ofdm_rx_hest, T4/estimate_channel.m:6,:8): the Task-4 receiver with
    mp_desync = 1 up to and including estimate_channel -- AutoCorrFunction, the two add_STO, add_CFO(-FreqOffset), remove_IFO, the
    demodulator, fine_sync, the pilot means, the spline -- on the route rx_chain_task4(time_desync, freq_desync, 1) takes; no
    equaliser, no demapper, no bits.

    rx: [(Nfft+Tg)*N_symb, n_frames] complex (numpy -> host flavour, torch.cuda -> device flavour).
    Returns dict(H_est=[n_frames, N_carrier] complex in the plan's precision with want_h, else None: bit for bit
    rx_chain_task4(..., mp_desync=1, want_h=True)["H"].T; Hest_at_pilots=[n_frames, Np] complex with want_pilots, else None:
    mean(rx(pilotCarriers,:) ./ pilotValues, 2) on the fine-synced symbols, the rows the spline reads; tg_position=[n_frames]
    int64, freq_offset=[n_frames] float64, ifo, status=[n_frames] int32: bit for bit that receiver's)."""
    call = _Call(rx, f64=plan.f64)
    rows, nfr = _shape2(rx)
    if rows != plan.frame_samples:
        raise OfdmError("rx_hest: rx must have (Nfft+T_guard)*N_symb rows")
    H, pH = (call.cout((plan.N_carrier, nfr)) if want_h else (None, None))                # memory [n_frames][N_carrier]
    Hp, pHp = (call.cout((plan.n_pilots, nfr)) if want_pilots else (None, None))
    tg, ptg = call._out((nfr,), np.int64, torch.int64 if call.dev else None)
    fo, pfo = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    ifo, pifo = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    stt, pst = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    L.check(call.lib.ofdm_rx_hest(plan.handle, call.cin(rx), nfr, int(time_desync), int(freq_desync), pH, pHp, ptg, pfo, pifo, pst,
                                  call.flags), "rx_hest")
    return dict(H_est=None if H is None else H.T, Hest_at_pilots=None if Hp is None else Hp.T, tg_position=tg, freq_offset=fo,
                ifo=ifo, status=stt)


_FINE_VARIANTS = {"T5": 0, "T4": 1}


def _error_specs(plan, n, frames, gap_bins, want_frames, want_map):
    """The outputs of the error anatomy for n points (n = None: one batch, no leading axis) as _outputs specs."""
    lead = () if n is None else (n,)
    gb = gap_bins if 1 <= gap_bins <= 1024 else 0                   # (a bad count is the library's refusal)
    u64 = lambda *shape: (lead + shape, np.uint64)
    return (u64(), u64(), u64(plan.n_data), u64(plan.N_symb), u64(plan.bps), u64(gb), u64(),
            (lead + (frames,), np.uint32) if want_frames else None, u64(plan.N_symb, plan.n_data) if want_map else None)


def _error_result(plan, on_device, frames, arrs):
    """The result of bit_error_profile / RxPlan.error_study from the arrays of _error_specs (`frames`: per point)."""
    err, fie, car, sym, lab, gap, above, fe, emap = arrs
    if not on_device:                                               # int64 views: a count of 2^63 is out of reach
        err, fie, car, sym, lab, gap, above = (a.view(np.int64) for a in (err, fie, car, sym, lab, gap, above))
        emap = None if emap is None else emap.view(np.int64)
        f64 = lambda a: a.astype(np.float64)
    else:
        f64 = lambda a: a.double()
    with np.errstate(divide="ignore", invalid="ignore"):            # no frame: NaN, the rate of nothing
        fer = f64(fie) / float(frames) if frames else f64(fie) * float("nan")
        cber = f64(car) / float(frames * plan.N_symb * plan.bps) if frames else f64(car) * float("nan")
    out = dict(errors=err, frames_in_error=fie, FER=fer, carrier_errors=car, carrier_BER=cber, dataCarriers=plan.dataCarriers.copy(),
               symbol_errors=sym, label_errors=lab, gap_hist=gap, gap_above=above, bits=frames * plan.frame_bits)
    if emap is not None:
        out["map"] = emap
    if fe is not None:
        out["frame_errors"] = fe
    return out


def bit_error_profile(plan: RxPlan, bits, ref_bits, gap_bins=64, want_map=False, want_frames=False):
    """Where the wrong bits of a batch of frames sit (ofdm_bit_error_profile).  bits, ref_bits: [n_frames, frame_bytes] uint8 packed
    as the receivers write bits= and read ref_bits_packed (both numpy -> host flavour, both torch.cuda -> device flavour, no host
    synchronisation).  Stream bit i of a frame has QAM index q = i // bps, label bit r = i % bps (0 = the MSB of the constellation
    label) and q = s * nd + d: OFDM symbol s, data carrier dataCarriers[d].  No receiver runs.
    Returns dict(errors (the wrong bits), frames_in_error, FER = frames_in_error / n_frames, carrier_errors=[nd], carrier_BER =
    carrier_errors / (n_frames * N_symb * bps), dataCarriers=[nd] (1-based, the axis of carrier_errors), symbol_errors=[N_symb],
    label_errors=[bps], gap_hist=[gap_bins], gap_above, bits = the bits compared (+ map=[N_symb, nd] with want_map)
    (+ frame_errors=[n_frames] uint32 with want_frames)), int64 counts.  For a frame's errors at stream positions i_0 < i_1 < .. the
    gaps are g_k = i_k - i_(k-1), within the frame only: gap_hist[g - 1] counts the gaps g <= gap_bins, gap_above the larger ones.
    Identities: sum(carrier_errors) = sum(symbol_errors) = sum(label_errors) = errors; sum(gap_hist) + gap_above = errors -
    frames_in_error; map.sum(0) = carrier_errors; map.sum(1) = symbol_errors.  Integers added in no particular order: the result
    does not depend on how the frames are spread over the device."""
    dev = _is_torch(bits) and bits.is_cuda
    if dev != (_is_torch(ref_bits) and ref_bits.is_cuda):
        raise OfdmError("bit_error_profile: bits and ref_bits must both be numpy arrays or both be CUDA tensors")
    if len(bits.shape) != 2 or bits.shape[1] != plan.frame_bytes or tuple(ref_bits.shape) != tuple(bits.shape):
        raise OfdmError("bit_error_profile: bits and ref_bits must be [n_frames, frame_bytes]")
    nfr = int(bits.shape[0])
    if dev:
        if bits.dtype != torch.uint8 or ref_bits.dtype != torch.uint8:
            raise OfdmError("bit_error_profile: bits and ref_bits must be uint8")
        b, r = bits.contiguous(), ref_bits.contiguous()
        pb, prf = C.c_void_p(b.data_ptr()), C.c_void_p(r.data_ptr())
        device = bits.device
    else:
        b = np.ascontiguousarray(np.asarray(bits.numpy() if _is_torch(bits) else bits, dtype=np.uint8))
        r = np.ascontiguousarray(np.asarray(ref_bits.numpy() if _is_torch(ref_bits) else ref_bits, dtype=np.uint8))
        pb, prf = b.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p)
        device = None
    arrs, ptrs, flags = plan._outputs(device, *_error_specs(plan, None, nfr, int(gap_bins), want_frames, want_map))
    L.check(plan.lib.ofdm_bit_error_profile(plan.handle, pb, prf, nfr, int(gap_bins), *ptrs, flags), "bit_error_profile")
    return _error_result(plan, dev, nfr, arrs)


def _fine_len(n_pilots, n_symb, variant):
    """numel(taus): Np * N_symb - 1 for T4/fine_sync.m when that is >= Np (:8 + :25-30), else Np * N_symb (the last entry 0)."""
    M = n_pilots * n_symb
    return M - 1 if variant == "T4" and M - 1 >= n_pilots else M


def rx_fine(plan: RxPlan, X, variant="T4", time_desync=1, want_taus=False, want_keep=False):
    """The fine synchroniser's curve of demodulated frames (ofdm_rx_fine): `taus` of T4/fine_sync.m:10-30 (variant="T5":
    T5/fine_sync.m:8-16), the residual delay every pair of adjacent pilots gives -- what figures 18a / 18b of the Task-4 report plot
    over the carrier number --, its mask (T4 :33, T5 :18) and the two estimates of fine_sync with their denominators.

    X: [Nfft, N_symb, n_frames] (or [Nfft, N_symb], one frame) complex, per frame what OFDM_demodulator returns and fine_sync takes
    (numpy -> host flavour, torch.cuda -> device flavour).  The pilots are the plan's.
    Returns dict(tau=[n_frames] float64, phase=[n_frames] float64 -- bit for bit fine_sync(frame, pilotCarriers, pilotValues,
    time_desync, ., variant, return_estimates=True)[1:], NaN = mean([]) --, n_used=[n_frames] int32 (the kept entries behind the
    first Np kept ones: the denominator of tau), n_phase=[n_frames] int32 (the angles above 1e-3: the denominator of phase),
    taus=[n_frames, L] float64 with want_taus (before the mask; L = Np N_symb - 1 for T4 when that is >= Np, else Np N_symb with a
    trailing 0), keep=[n_frames, L] uint8 with want_keep, else None)."""
    if variant not in _FINE_VARIANTS:
        raise OfdmError("rx_fine: variant must be 'T4' or 'T5'")
    call = _Call(X, f64=plan.f64)
    shape = tuple(X.shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[:2] != (plan.Nfft, plan.N_symb):
        raise OfdmError("rx_fine: X must be [Nfft, N_symb, n_frames]")
    nfr = int(shape[2])
    Lt = _fine_len(plan.n_pilots, plan.N_symb, variant)
    taus, ptaus = (call._out((nfr * Lt,), np.float64, torch.float64 if call.dev else None) if want_taus else (None, None))
    keep, pkeep = (call._out((nfr * Lt,), np.uint8, torch.uint8 if call.dev else None) if want_keep else (None, None))
    tau, ptau = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    ph, pph = call._out((nfr,), np.float64, torch.float64 if call.dev else None)
    nu, pnu = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    nph, pnph = call._out((nfr,), np.int32, torch.int32 if call.dev else None)
    L.check(call.lib.ofdm_rx_fine(plan.handle, call.cin(X), nfr, _FINE_VARIANTS[variant], int(bool(time_desync)), ptaus, pkeep, ptau,
                                  pph, pnu, pnph, call.flags), "rx_fine")
    return dict(tau=tau, phase=ph, n_used=nu, n_phase=nph, taus=None if taus is None else taus.reshape(nfr, Lt),
                keep=None if keep is None else keep.reshape(nfr, Lt))


def _mer_db(sums):
    """10 log10(s1 / s2) of [..., 2] MER_func sums (T5/MER_func.m:25): on the device for a torch tensor, no synchronisation."""
    if _is_torch(sums):
        return 10.0 * torch.log10(sums[..., 0] / sums[..., 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        return 10.0 * np.log10(sums[..., 0] / sums[..., 1])


def task5_part2_tile(plan: RxPlan, tx_noised, taps_list, SNR_dB, ref_bits_packed):
    """One tile of T5/Task5_part2.m:148-205, :269-304: every channel realisation of `taps_list` (each a [(delay, amplitude)]
    array like `channel_taps`, all of the same length) applied to the scenario's noisy TX stream `tx_noised`, then LS_CE,
    MMSE_CE (h = the true CIR, SNR_dB), MP_estimate and OMP_estimate (dominant_taps = the plan's), their NMSE against
    fft(h) and the four equalise / demap / BER passes -- one device-resident pass, only the sums come back.

    ref_bits_packed: the scenario's payload, ONE packed frame [frame_bytes] (every realisation shares the TX frame).
    Returns dict(nmse=[4, n] float64, errors=[4, n] uint32) with rows LS, MMSE, MP, OMP."""
    call = _Call(tx_noised, f64=plan.f64)
    n = len(taps_list)
    T = np.asarray(taps_list[0]).shape[0] if n else 1
    delay = np.zeros((max(n, 1), T), dtype=np.int32)                  # (an empty tile still hands the entry valid pointers)
    amp = np.zeros((max(n, 1), T), dtype=np.complex128)
    for i, t in enumerate(taps_list):
        t = np.asarray(t)
        if t.shape[0] != T:
            raise OfdmError("task5_part2_tile: every realisation needs the same number of channel taps")
        delay[i] = np.real(t[:, 0]).astype(np.int32)
        amp[i] = t[:, 1]
    ref = ref_bits_packed
    ref = ref.contiguous().view(-1) if _is_torch(ref) else np.ascontiguousarray(ref).reshape(-1)
    if ref.shape[0] != plan.frame_bytes:
        raise OfdmError("task5_part2_tile: ref_bits_packed must be one packed frame")
    pref = call._flat(ref, np.uint8, torch.uint8 if call.dev else None)[0]
    nm, pnm = call._out((n, 4), np.float64, torch.float64 if call.dev else None)      # memory [4][n]
    er, per = call._out((n, 4), np.uint32, torch.int32 if call.dev else None)
    ampv = np.ascontiguousarray(amp).view(np.float64)
    if n == 0:
        pnm = call._out((1, 4), np.float64, torch.float64 if call.dev else None)[1]
        per = call._out((1, 4), np.uint32, torch.int32 if call.dev else None)[1]
    L.check(call.lib.ofdm_task5_part2_tile(plan.handle, call.cin(tx_noised), C.c_void_p(delay.ctypes.data),
                                           C.c_void_p(ampv.ctypes.data), T, n, float(SNR_dB), pref, pnm, per, call.flags),
            "task5_part2_tile")
    return dict(nmse=nm.T, errors=er.T)


def task5_mse_tile(plan: RxPlan, Tx, channel_taps, SNRs, seed=0, stream0=0):
    """One tile of the MSE(SNR) sweep of T5/Main_model_Task_5.m:303-346 (ofdm_task5_mse_tile): for every SNR of `SNRs`
    Noise(SNR, Tx) (Philox stream stream0 + i) -> conv(h) truncated -> OFDM_demodulator -> LS_CE, MMSE_CE(h = ifft(H_LS), SNR),
    MP_estimate, OMP_estimate -> mean squared error against fft(h) on 1..N_carrier.  Tx: the clean TX stream of one frame
    (numpy -> host flavour, torch.cuda -> device flavour); channel_taps: [(delay, amplitude)] rows like the script's.
    Returns MSEs [4, n] float64, rows LS, MMSE, MP, OMP."""
    call = _Call(Tx, f64=plan.f64)
    t = np.asarray(channel_taps)
    delay = np.ascontiguousarray(np.real(t[:, 0]).astype(np.int32))
    amp = np.ascontiguousarray(t[:, 1].astype(np.complex128)).view(np.float64)
    snr = np.ascontiguousarray(np.asarray(SNRs, dtype=np.float64).ravel())
    n = snr.size
    ms, pms = call._out((n, 4), np.float64, torch.float64 if call.dev else None)      # memory [4][n]
    L.check(call.lib.ofdm_task5_mse_tile(plan.handle, call.cin(Tx), C.c_void_p(delay.ctypes.data), C.c_void_p(amp.ctypes.data),
                                         delay.size, C.c_void_p(snr.ctypes.data), n, int(seed), int(stream0), pms, call.flags),
            "task5_mse_tile")
    return ms.T


_OMP_ROUTES = {"auto": 0, "batch": 1, "wide": 2}
_OMP_ROUTE_NAMES = {v: k for k, v in _OMP_ROUTES.items()}


def OMP_estimate_batch(plan: RxPlan, Y, route="auto", want_h=False):
    """T5/OMP_estimate.m:7-23 for every column of Y [Np, n] against the plan's dictionary (ofdm_OMP_estimate_batch): the OMP
    step of task5_part2_tile / task5_mse_tile on its own.  route: "auto" (omp_batch_kernel while its state fits the LDS, else
    the wide kernel), "batch" or "wide" to force one; a route that cannot serve the shape raises OfdmError.
    Returns (index [taps, n] int32, 1-based picks in pick order, 0 = not made; x [taps, n] complex128, the picks' coefficients;
    H [N_carrier, n] in the plan's precision, or None without want_h)."""
    if route not in _OMP_ROUTES:
        raise OfdmError(f"OMP_estimate_batch: route must be one of {sorted(_OMP_ROUTES)}")
    call = _Call(Y, f64=plan.f64)
    npil, n = _shape2(Y)
    if npil != plan.n_pilots:
        raise OfdmError("OMP_estimate_batch: Y needs one row per pilot of the plan")
    T = plan.taps
    idx, pidx = call._out((T, n), np.int32, torch.int32 if call.dev else None)
    x, px = call._out((T, n), np.complex128, torch.complex128 if call.dev else None)
    H, pH = call.cout((plan.N_carrier, n)) if want_h else (None, None)
    L.check(call.lib.ofdm_OMP_estimate_batch(plan.handle, call.cin(Y), n, _OMP_ROUTES[route], pidx, px, pH, call.flags),
            "OMP_estimate_batch")
    return idx, x, H
