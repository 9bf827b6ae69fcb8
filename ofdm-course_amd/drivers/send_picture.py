"""What every driver of the reference does before its curves: a picture's bits through the chain and back.

`file_reader.m` reads a picture and binarises it, the chain carries its bits, the DeScrambler returns them, "Проверка пройдена!" is
printed when they are the bits that went in, and `display_pic.m` shows the received picture (`Task 3/Main_model_Task_3.m:26-32`,
`:160-185`; the same lines in the other four drivers).  Here the whole of it is one device-resident call per run,
`RxPlan.transport` (ofdm_payload_transport): the payload at every SNR point, `--repeats` times, decoded by the Task-5 or the Task-4
receiver, the received stream, the error counts and the per-bit sums back as integers.

    python -m ofdm_course_amd.drivers.send_picture --json out.json [--file PATH | --card] [--snr 5,10,15,25]
        [--config T3|T4|T5|M|small] [--receiver task5|task4] [--fading EPA] [--repeats N] [--pgm-dir DIR]

  --file   any file: its bytes are the payload, MSB first.  A `.pgm` (P5) or `.npy` image is binarised at half scale and read
           column-major, as imbinarize and (:) do (file_reader.m:6-10).  No image library is needed; TIFF is not read.
  --card   (the default) a 360 x 360 test card built in numpy -- a border, bars and a disc -- with enough structure that a burst of
           errors is visible.
  --pgm-dir  per point the first repeat's picture and the mean picture (ones / repeats) as P5 files laid out as display_pic.m
           lays them: 360 x 360 column-major, zero-padded, x 255.

The link: the Register of T3:36 on both ends and the 3-tap channel of T3:122-126, or with --fading a channel realisation per frame
on a 3GPP delay line.  Under `python -m torch.distributed.run` the repeats are dealt to the ranks through frame0 (repeat r is the
Philox streams frame0 + r F ..), and one int64 all-reduce joins the counts; the pictures are rank 0's repeats.
"""
from __future__ import annotations

import argparse
import json
import os

import numpy as np

from .. import frames as fr
from .. import sweep
from . import common as c

SIDE = 360                                                                        # display_pic.m:5-9
T3_TAPS = np.array([[0, 1.0], [2, 0.4], [4, 0.01]])                               # T3/Main_model_Task_3.m:122-126
CONFIGS = ("T3", "T4", "T5", "M", "small")


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


# ---- pictures and bits (host bookkeeping, no signal arithmetic)
def test_card():
    """[360, 360] uint8 of 0 / 1: a border, vertical bars of growing width, horizontal stripes and a disc."""
    y, x = np.mgrid[0:SIDE, 0:SIDE]
    img = np.zeros((SIDE, SIDE), np.uint8)
    img[(x < 8) | (x >= SIDE - 8) | (y < 8) | (y >= SIDE - 8)] = 1
    bars = (y >= 24) & (y < 120) & (x >= 24) & (x < SIDE - 24)
    img[bars & ((np.floor(np.sqrt(np.maximum(x - 24, 0) * 4.0)).astype(int) % 2) == 0)] = 1
    img[(y >= 136) & (y < 200) & (x >= 24) & (x < SIDE - 24) & ((y // 4) % 2 == 0)] = 1
    img[(x - 180) ** 2 + (y - 272) ** 2 < 56 ** 2] = 1
    img[(x - 180) ** 2 + (y - 272) ** 2 < 24 ** 2] = 0
    return img


def binarize(gray):
    """imbinarize at half scale (file_reader.m:6): above half of the type's range (or of the largest value of a float image)."""
    g = np.asarray(gray)
    if g.ndim == 3:
        g = g.mean(axis=2)
    top = float(np.iinfo(g.dtype).max) if g.dtype.kind in "ui" else float(max(g.max(), 1e-300))
    return (g.astype(np.float64) > top / 2).astype(np.uint8)


def image_bits(img01):
    """binaryImage(:) (file_reader.m:7-10): column-major."""
    return np.asarray(img01, np.uint8).ravel(order="F")


def read_pgm(path):
    """A binary PGM (P5), 8 or 16 bits -> [height, width]."""
    with open(path, "rb") as f:
        data = f.read()
    tokens, at = [], 0
    while len(tokens) < 4:
        while data[at:at + 1].isspace():
            at += 1
        if data[at:at + 1] == b"#":
            at = data.index(b"\n", at)
            continue
        end = at
        while not data[end:end + 1].isspace():
            end += 1
        tokens.append(data[at:end])
        at = end
    if tokens[0] != b"P5":
        raise ValueError(f"{path}: not a binary PGM (P5)")
    w, h, maxval = int(tokens[1]), int(tokens[2]), int(tokens[3])
    dt = np.dtype(">u2") if maxval > 255 else np.dtype(np.uint8)
    img = np.frombuffer(data, dt, count=w * h, offset=at + 1).reshape(h, w)
    return (img.astype(np.float64) > maxval / 2).astype(np.uint8)


def read_payload(path):
    """-> (bits, what it was read as)."""
    low = path.lower()
    if low.endswith(".pgm"):
        return image_bits(read_pgm(path)), "pgm"
    if low.endswith(".npy"):
        return image_bits(binarize(np.load(path))), "npy"
    with open(path, "rb") as f:
        return np.unpackbits(np.frombuffer(f.read(), np.uint8)), "bytes"


def picture(bits):
    """display_pic.m:5-12: the bits zero-padded (or cut) to 360 x 360, column-major, x 255."""
    b = np.zeros(SIDE * SIDE, np.uint8)
    n = min(b.size, np.asarray(bits).size)
    b[:n] = np.asarray(bits, np.uint8).ravel()[:n]
    return b.reshape((SIDE, SIDE), order="F") * np.uint8(255)


def mean_picture(ones, repeats):
    """The mean received picture of a point: round(255 ones / repeats), laid out as picture()."""
    b = np.zeros(SIDE * SIDE, np.float64)
    n = min(b.size, np.asarray(ones).size)
    b[:n] = np.asarray(ones, np.float64).ravel()[:n]
    return np.floor(255.0 * b / float(repeats) + 0.5).astype(np.uint8).reshape((SIDE, SIDE), order="F")


def write_pgm(path, img):
    img = np.ascontiguousarray(img, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


def snr_tag(snr):
    return ("%g" % snr).replace("-", "m").replace(".", "p")


# ---- the link
def link(config):
    """-> (FrameConfig, channel taps, Register) of a named configuration: the frame of the named driver (T3 / T4: T3:6-27 with the
    percent pilot rule; T5: T5:6-38; M: frames.config_M; small: frames.config_small), the 3-tap channel of T3:122-126."""
    if config in ("T3", "T4"):
        _, pil, _ = c.layout_percent(1024, 400, 15, tail=2)
        cfg = fr.FrameConfig(config, 1024, 400, 6, "16QAM", N_symb=5, taps=T3_TAPS.copy(), dominant_taps=3, pilots=pil, pilot_amp=4 / 3,
                             K_atoms=int(np.ceil(400 / 6)))
    elif config == "T5":
        cfg = fr.FrameConfig("T5", 4096, 1024, 4, "16QAM", N_symb=7, taps=T3_TAPS.copy(), dominant_taps=3)
    elif config == "M":
        cfg = fr.config_M()
        cfg.taps, cfg.dominant_taps = T3_TAPS.copy(), 3
    elif config == "small":
        cfg = fr.config_small(taps=T3_TAPS.copy())
    else:
        raise ValueError(f"send_picture: config must be one of {CONFIGS}")
    return cfg, T3_TAPS, c.REGISTER


def my_repeats(repeats, rank, world):
    """The repeats dealt to this rank: (first, count), a partition of 0 .. repeats - 1 in order."""
    base, extra = divmod(repeats, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def reduce_counts(counts, device=None):
    """The one collective of a run: an int64 block through sweep.all_reduce_counters (a no-op on one rank)."""
    box = sweep.Counters(*counts.shape)
    box.errors += counts
    return sweep.all_reduce_counters(box, device=device).errors


def run(bits, snrs=(5.0, 10.0, 15.0, 25.0), config="T3", receiver="task5", fading=None, repeats=1, seed=1, precision="fp32",
        device_index=0, lib=None, rank=0, world=1, reduce=reduce_counts, pgm_dir=None, make_plan=None):
    """Returns (on every rank) dict(n_bits, frames, SNR_dB, errors [n_points][repeats], BER, loopback, ...).  lib: the library
    module (default: ofdm_course_amd); make_plan(cfg, lib, precision, device_index): a stand-in for frames.make_plan (tests)."""
    if lib is None:
        import ofdm_course_amd as lib
    lib.init(device_index)
    bits = np.asarray(bits, np.uint8).ravel()
    snrs = [float(s) for s in snrs]
    if repeats < 1 or bits.size < 1 or not snrs:
        raise ValueError("send_picture: a payload of at least one bit, at least one SNR and repeats >= 1 are needed")
    cfg, taps, reg = link(config)
    plan = (make_plan or (lambda cf, lb, pr, di: fr.make_plan(cf, lb, precision=pr, device=di)))(cfg, lib, precision, device_index)
    plan.set_descrambler(reg)
    kw = dict(receiver=receiver, Register=reg, seed=seed, want_ones=True)
    if fading is not None:
        kw["fading"] = c.fading_profile(fading, 15e3 * cfg.Nfft)
    else:
        kw["h"] = lib.get_MP_channel_resp(taps, cfg.Nfft)[0]
    F = -(-bits.size // plan.frame_bits)
    first, count = my_repeats(repeats, rank, world)
    n = len(snrs)
    block = np.zeros((n, repeats + bits.size), np.int64)                          # [errors of every repeat | ones]
    first_bits = None
    if count:
        out = plan.transport(bits, snrs, repeats=count, frame0=first * F, **kw)
        block[:, first:first + count] = _np(out["errors"])
        block[:, repeats:] = _np(out["ones"])
        first_bits = _np(out["decoded_bits"])[:, 0]
    plan.close()
    block = np.asarray(reduce(block))
    errors, ones = block[:, :repeats], block[:, repeats:]
    res = {"driver": "Task 3/Main_model_Task_3.m:26-32,:160-185, file_reader.m, display_pic.m", "config": config, "receiver": receiver,
           "fading": fading, "n_bits": int(bits.size), "frame_bits": int(plan.frame_bits), "frames": int(F), "repeats": int(repeats),
           "seed": int(seed), "dtype": "f32" if precision == "fp32" else "f64", "n_gpus": world, "SNR_dB": snrs,
           "errors": errors, "BER": errors / np.float64(bits.size), "loopback": errors == 0,
           "bit_error_rate_of_the_mean_picture": np.abs(ones / np.float64(repeats) - bits[None, :]).mean(axis=1)}
    if pgm_dir is not None and rank == 0:
        os.makedirs(pgm_dir, exist_ok=True)
        for p, snr in enumerate(snrs):
            if first_bits is not None:
                write_pgm(os.path.join(pgm_dir, f"snr_{snr_tag(snr)}_first.pgm"), picture(first_bits[p]))
            write_pgm(os.path.join(pgm_dir, f"snr_{snr_tag(snr)}_mean.pgm"), mean_picture(ones[p], repeats))
    return res


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group()
    src.add_argument("--file", default=None, help="the payload: any file's bytes; .pgm (P5) and .npy images are binarised")
    src.add_argument("--card", action="store_true", help="the 360 x 360 test card (the default)")
    ap.add_argument("--snr", default="5,10,15,25", help="SNR points in dB, comma separated")
    ap.add_argument("--config", choices=CONFIGS, default="T3")
    ap.add_argument("--receiver", choices=["task5", "task4"], default="task5")
    ap.add_argument("--fading", choices=sorted(c.DELAY_PROFILES), default=None, help="a channel per frame on this 3GPP delay line")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--precision", choices=["fp32", "fp64"], default="fp32")
    ap.add_argument("--pgm-dir", default=None)
    ap.add_argument("--backend", default="nccl", help="nccl = RCCL over xGMI; gloo for rehearsals")
    ap.add_argument("--device", type=int, default=None, help="the GPU of this process (default: its local rank)")
    ap.add_argument("--json", default=None)
    return ap


def main(argv=None, lib=None, make_plan=None):
    """One process per GPU (RANK / LOCAL_RANK / WORLD_SIZE of torch.distributed.run); rank 0 writes the result.  lib / make_plan:
    stand-ins for the library (tests): one rank, no process group."""
    ap = parser()
    a = ap.parse_args(argv)
    try:
        snrs = [float(s) for s in a.snr.split(",") if s.strip()]
    except ValueError:
        ap.error("--snr must be numbers separated by commas")
    if not snrs or a.repeats < 1:
        ap.error("at least one SNR and --repeats >= 1 are needed")
    bits, source = (image_bits(test_card()), "card") if a.file is None else read_payload(a.file)
    rank, local_rank, world = (0, 0, 1) if lib is not None else sweep.dist_env()
    dev_index = local_rank if a.device is None else a.device
    reduce = reduce_counts
    if world > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(dev_index)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if a.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
            reduce = lambda counts: reduce_counts(counts, device=torch.device("cuda", dev_index))  # noqa: E731
        else:
            dist.init_process_group(a.backend)
    res = run(bits, snrs, a.config, a.receiver, a.fading, a.repeats, a.seed, a.precision, device_index=dev_index, lib=lib, rank=rank,
              world=world, reduce=reduce, pgm_dir=a.pgm_dir, make_plan=make_plan)
    res["source"] = source
    if rank == 0:
        text = json.dumps(c.to_jsonable(res))
        if a.json:
            with open(a.json, "w") as f:
                f.write(text)
        else:
            print(text, flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
