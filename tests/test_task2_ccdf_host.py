"""drivers/task2_ccdf.py on the CPU: its argument checks, the grid parser, the cyclic payload reader and the dealing of the
signals to the ranks.  Nothing here touches a GPU."""
import os

import numpy as np
import pytest

from ofdm_course_amd import sweep
from ofdm_course_amd.drivers import task2_ccdf as t2c

HERE = os.path.dirname(os.path.abspath(__file__))
EAGLE = os.path.join(HERE, "golden", "eagle_bits.npz")
GRID = dict(n=600, lo=0.0, hi=30.0)


def test_bins_parser():
    assert t2c.parse_bins("600,0,30") == GRID
    assert t2c.parse_bins("1200,-2.5,1e1") == dict(n=1200, lo=-2.5, hi=10.0)
    for bad in ("600", "600,0", "600,0,30,1", "x,0,30", "600,a,30", "6.5,0,30"):
        with pytest.raises(ValueError):
            t2c.parse_bins(bad)


def test_argument_checks_each_have_their_text():
    assert t2c.check_args(8, 10, "random", GRID) is None
    assert t2c.check_args(1, 1, EAGLE, dict(n=1, lo=-1.0, hi=0.0), 1) is None
    assert t2c.check_args(0, 10, "random", GRID) == "--signals must be >= 1"
    assert t2c.check_args(8, 0, "random", GRID) == "--frames-per-signal must be >= 1"
    assert t2c.check_args(8, 10, "random", GRID, 0) == "--signals-per-tile must be >= 1"
    assert t2c.check_args(8, 10, "random", dict(GRID, n=0)) == "--bins: N must be 1 .. 4096"
    assert t2c.check_args(8, 10, "random", dict(GRID, n=4097)) == "--bins: N must be 1 .. 4096"
    for lo, hi in ((30.0, 30.0), (5.0, 1.0), (float("-inf"), 1.0), (0.0, float("nan"))):
        assert t2c.check_args(8, 10, "random", dict(n=10, lo=lo, hi=hi)) == "--bins: LO and HI must be finite with LO < HI"
    assert t2c.check_args(8, 10, "image.tiff", GRID) == "--payload must be 'random' or a .npz file"
    assert t2c.check_args(8, 10, "/nowhere/x.npz", GRID) == "--payload: /nowhere/x.npz not found"
    # the first failing check is the one reported
    assert t2c.check_args(0, 0, "image.tiff", dict(GRID, n=0)) == "--signals must be >= 1"


def test_command_line(capsys):
    a = t2c.parse_args(["--signals", "16", "--frames-per-signal", "3", "--bins", "100,2,12", "--payload", EAGLE])
    assert (a.signals, a.frames_per_signal, a.bins, a.payload, a.json) == (16, 3, dict(n=100, lo=2.0, hi=12.0), EAGLE, None)
    d = t2c.parse_args([])
    assert (d.signals, d.frames_per_signal, d.bins, d.payload, d.precision) == (1024, 10, GRID, "random", "fp64")   # T2:9-11
    for argv, text in ((["--signals", "0"], "--signals must be >= 1"), (["--bins", "5,3"], "--bins must be N,LO,HI"),
                       (["--bins", "0,0,1"], "--bins: N must be 1 .. 4096"), (["--payload", "x.tiff"], "--payload must be")):
        with pytest.raises(SystemExit):
            t2c.parse_args(argv)
        assert text in capsys.readouterr().err
    with pytest.raises(ValueError, match="--frames-per-signal"):
        t2c.run(signals=4, frames_per_signal=0)                          # refused before the device is touched


def test_payload_file_is_read_cyclically():
    bits = t2c.load_payload(EAGLE)
    g = np.load(EAGLE)
    assert bits.size == int(g["n_bits"]) and set(np.unique(bits)) <= {0, 1}
    per = 1000
    a = t2c.signal_bits(bits, 0, 3, per)
    assert a.shape == (3, per) and np.array_equal(a.ravel(), bits[:3000])
    # signal i is the same bits whichever tile it is dealt in, and the file wraps around
    b = t2c.signal_bits(bits, 2, 2, per)
    assert np.array_equal(b[0], a[2])
    last = bits.size // per
    w = t2c.signal_bits(bits, last, 1, per)[0]
    assert np.array_equal(w, np.concatenate([bits[last * per:], bits[:per - (bits.size - last * per)]]))


def test_the_docstring_says_what_the_scrambler_is_for():
    doc = t2c.__doc__
    assert "the two curves coincide" in doc and "structured payload" in doc and "T2:36" in doc


def test_signals_are_dealt_as_a_partition():
    """The tiles of run(): ceil(signals / signals_per_tile) of them, dealt by sweep.tiles_for_rank, every signal exactly once."""
    signals, per_tile = 37, 5
    n_tiles = -(-signals // per_tile)
    for world in (1, 2, 3, 8):
        seen = []
        for rank in range(world):
            for _, b in sweep.tiles_for_rank(1, n_tiles, rank, world):
                s0 = b * per_tile
                seen += list(range(s0, s0 + min(per_tile, signals - s0)))
        assert sorted(seen) == list(range(signals))
