"""The sharded BER(SNR) sweep (drivers/sweep_ber.py): two gloo ranks sharing the one GPU of the test box must
reproduce the single-process table exactly (integer counters, tile-keyed noise streams)."""
import hashlib
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, out):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(out) as f:
        return json.load(f)


@pytest.mark.parametrize("config,estimator", [("M", "omp"), ("C5", "omp"), ("M", "mmse")])
def test_two_rank_sweep_equals_single_process(tmp_path, config, estimator):
    common = ["--config", config, "--estimator", estimator, "--batches", "2", "--frames-per-tile", "3",
              "--snrs", "4", "16", "28"]
    one = _run([sys.executable, "-m", "ofdm_course_amd.drivers.sweep_ber", *common, "--json", str(tmp_path / "one.json")],
               tmp_path / "one.json")
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                "127.0.0.1", "--master-port", str(_free_port()), "-m", "ofdm_course_amd.drivers.sweep_ber", *common,
                "--backend", "gloo", "--force-device", "0", "--json", str(tmp_path / "two.json")], tmp_path / "two.json")
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert one["errors"] == two["errors"] and one["bits"] == two["bits"]
    assert one["BER"][0] > one["BER"][-1] >= 0.0
    assert sum(one["bits"]) > 0


def _bench(*argv):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus 2` as a bare command (no torch.distributed.run): the parent spawns the two ranks itself
    (here both on GPU 0 over gloo).  Weak scaling with global frame ids: 2 ranks x 512 frames decode exactly the frames
    of 1 rank x 1024, so the per-frame error digest is the same."""
    two = _bench("--gpus", "2", "--backend", "gloo", "--force-device", "0", "--steps", "5", "--warmup", "2",
                 "--frames", "512", "--no-cpu")
    one = _bench("--gpus", "1", "--steps", "5", "--warmup", "2", "--frames", "1024", "--full", "--no-cpu", "--no-secondary",
                 "--f64-steps", "3")
    # the single-GPU line carries the reference-precision leg (fp64 plan, the same chain entry) and the environment in force
    assert one["f64"]["dtype"] == "f64" and one["f64"]["value"] > 0 and 0 < one["f64"]["roofline"]["frac"] < 1
    assert isinstance(one["env"], dict) and "f64" not in two
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1 and two["steps"] == 5
    assert two["frame_errors"] == one["frame_errors"] and one["frame_errors"]["frames"] == 1024
    assert two["config"]["symbols_per_step"] == one["config"]["symbols_per_step"] == 1024 * 14
    assert two["scaling"] == "weak" and two["value"] > 0 and "roofline" in two


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline line without the legs that take runs of their own, and --dump-outputs
    writes what the last timed step returned: per-frame error counts (every frame) and packed decided bits (a seeded
    sample), float32, identical in two runs with the same arguments."""
    argv = ("--gpus", "1", "--steps", "4", "--warmup", "1", "--frames", "1024")
    a = _bench(*argv, "--dump-outputs", str(tmp_path / "a"))
    b = _bench(*argv, "--dump-outputs", str(tmp_path / "b"))
    for r in (a, b):
        assert r["steps"] == 4 and r["ms_per_step"] > 0 and r["value"] > 0 and r["dtype"] == "f32"
        assert r["higher_is_better"] is True and r["unit"] == "OFDM symbols/s" and "roofline" in r
        assert not {"kernels_ms", "roofline_dominant", "cpu_baseline", "ber_match", "f64", "secondary"} & set(r)
    assert a["frame_errors"] == b["frame_errors"]
    got = {}
    for name in ("errors", "bits"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, y), name
        got[name] = x
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    errs = got["errors"].astype(np.int32)
    assert errs.shape == (1024,) and np.array_equal(errs, got["errors"])
    assert hashlib.sha1(errs.astype("<i4").tobytes()).hexdigest() == a["frame_errors"]["sha1"]
    bits = got["bits"]
    assert bits.shape[0] == 1024 and bits.min() >= 0 and bits.max() <= 255 and np.array_equal(bits, np.round(bits))
