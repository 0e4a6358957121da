"""bench.py's result line and --dump-outputs on a small config-4-shaped model: a plain run prints
the headline figure only, writes the record of its last timed sweep (the same arrays Chain.run
hands a caller that repeats the benchmark's sweeps), and does so identically from run to run;
--full adds the other measurements to the same line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import H, ROOT
from hmsc_amd.workloads import synthetic_probit

pytestmark = pytest.mark.gpu

BENCH = os.path.join(ROOT, "bench.py")
SIZE = dict(ny=301, ns=41, nc=4, nf=3)          # odd sizes, no multiple of a tile
STEPS, WARMUP, RAMP = 6, 3, 70                   # the ramp runs one block of 50 and one of 20
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("beta_ess_per_s", "roofline", "kernels_eager_events_us", "cpu_baseline", "sharded_chain")


def _bench(extra):
    args = ["--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP), "--clock-warmup-sweeps", str(RAMP)]
    for k, v in SIZE.items():
        args += [f"--{k}", str(v)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH] + args + extra, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench(["--dump-outputs", str(d)]), d


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_line_is_the_headline(plain):
    res, _ = plain
    for k in HEADLINE:
        assert k in res, k
    for k in FULL_ONLY:
        assert k not in res, k
    assert res["steps"] == STEPS and res["warmup"] == WARMUP and res["clock_warmup_sweeps"] == RAMP
    assert res["unit"] == "sweeps/s" and res["higher_is_better"] is True and res["dtype"] == "f64"
    assert res["ms_per_step"] > 0
    # value is the rate of the same timed region ms_per_step describes (both rounded in the line)
    assert res["value"] == pytest.approx(1e3 / res["ms_per_step"], rel=1e-2)
    # the in-kernel timer saw exactly the timed sweeps
    assert res["graphs_prebuilt"] is True and res["kernels_live_us"]["z"] > 0


def test_dump_is_the_last_timed_sweep(plain):
    """The benchmark's sweeps repeated through the package: the dumped arrays are that run's
    record at its last sample, bit for bit (every draw is keyed by seed and sweep number)."""
    _, d = plain
    got = _load(d)
    hM = synthetic_probit(**SIZE)
    ch = H.Chain(hM, 1234567, device=0, updater={"GammaEta": False})
    ch.init([SIZE["nf"]])
    ch.kernel_timing(True)
    ch.run(transient=0, samples=1, thin=1, adaptNf=[0], record=True)
    ch.prepare_graphs(2)
    it = 1
    for n in (WARMUP - 1, 50, RAMP - 50):        # the rest of the warm-up, then the ramp's blocks
        ch.run(transient=0, samples=n, thin=1, adaptNf=[0], iter0=it, record=True)
        it += n
    assert it == WARMUP + RAMP
    rec = ch.run(transient=0, samples=STEPS, thin=1, adaptNf=[0], iter0=it, record=True)
    ch.close()
    assert sorted(got) == sorted(rec)
    nbytes = 0
    for name, a in got.items():
        assert a.dtype == np.float64, name
        nbytes += a.nbytes
        want = rec[name][:, -1] if name == "nf" else rec[name][-1]
        np.testing.assert_array_equal(a, np.asarray(want, dtype=np.float64), err_msg=name)
    assert got["Beta"].shape == (SIZE["nc"], SIZE["ns"]) and got["Eta0"].shape == (SIZE["ny"], SIZE["nf"])
    assert nbytes <= 64 << 20


def test_second_run_dumps_the_same(plain, tmp_path):
    _, d = plain
    _bench(["--dump-outputs", str(tmp_path)])
    a, b = _load(d), _load(tmp_path)
    assert sorted(a) == sorted(b)
    for name in a:
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)


def test_full_adds_the_other_measurements():
    # (without the species-sharded leg, which adds ~9 s at any model size: an RCCL communicator
    # and at least 200 timed sweeps after 0.5 s of warm-up; tests/test_gpu_sharded.py runs that chain)
    res = _bench(["--full", "--ess-samples", "1000", "--cpu-sweeps", "1", "--no-sharded-leg"])
    for k in HEADLINE + FULL_ONLY:
        assert k in res, k
    assert res["beta_ess_per_s"]["n_beta"] == SIZE["nc"] * SIZE["ns"] and res["beta_ess_per_s"]["median"] > 0
    assert res["roofline"]["kernel"] in ("z", "eta", "betalambda") and res["roofline"]["avg_launch_us"] > 0
    assert res["kernels_eager_events_us"]["sweep"] > 0
    assert res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["kind"] == "port"
    assert res["sharded_chain"] is None
