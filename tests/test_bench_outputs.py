"""bench.py's lean default run, --dump-outputs and --full: the plain line carries the headline only, the dumps are
the ten results of the timed path on seeded inputs (the same from run to run), and --full still adds the CPU
baseline, the parity check and the other shapes."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vtem", "omegatem", "wtem", "psitem", "epfy", "epfz", "epdiv", "utendepfd", "utendvtem", "utendwtem")
NE, NLEV, NT = 8, 12, 5
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "ne%dx%dx%d" % (NE, NLEV, NT)]


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=timeout, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_samples_a_large_result_the_same_way_every_time(tmp_path, monkeypatch):
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 10 * 8 * 1000)          # 1000 float64 values per result
    res = np.random.default_rng(3).standard_normal((10, 20, 7, 11))        # 1540 values per result: sampled
    bench.dump_outputs(str(tmp_path / "a"), NAMES, torch.from_numpy(res))
    bench.dump_outputs(str(tmp_path / "b"), NAMES, torch.from_numpy(res.astype(np.float32)))
    total = 0
    for i, n in enumerate(NAMES):
        a = np.load(str(tmp_path / "a" / (n + ".npy")))
        b = np.load(str(tmp_path / "b" / (n + ".npy")))
        assert a.dtype == np.float64 and a.shape == (1000,) and b.shape == (1000,)
        assert np.all(np.isin(a, res[i]))                                    # values of the result, not made up
        assert np.array_equal(b, a.astype(np.float32).astype(np.float64))   # the same positions for the same shape
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    small = res[:, :5, :3, :2]                                               # under the limit: dumped whole
    bench.dump_outputs(str(tmp_path / "c"), NAMES, torch.from_numpy(small))
    assert np.array_equal(np.load(str(tmp_path / "c" / "epdiv.npy")), small[6])


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run: the headline fields, exactly --steps timed steps, none of the --full extras; the dumps equal the
    engine's results on the same seeded inputs, and a second run dumps the same bits."""
    import torch
    from pytemdiags_amd import _lib, engine, synth
    rec = _run(SMALL + ["--dump-outputs", str(tmp_path / "d1")])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "grid-points/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    assert rec["metric"].startswith("grid-points/sec through full TEM pipeline") and not rec["nonfinite"]
    for k in ("cpu_baseline", "parity_vs_oracle_on_sample", "other_workloads", "roofline"):
        assert k not in rec, k
    assert sorted(os.listdir(str(tmp_path / "d1"))) == sorted(n + ".npy" for n in NAMES)
    lat, lon = synth.cubed_sphere_gll(NE, mirror=False)
    plev = synth.pressure_levels(NLEV)
    zm = (np.arange(-90, 91, 1.0)[1:] + np.arange(-90, 91, 1.0)[:-1]) / 2
    plan = engine.Plan(lat, zm, 50, device=0)
    plan.set_tem(NLEV, NT, plev * 100)
    f = engine.synth_fields(0, lat, lon, plev, NT, dtype=torch.float64, seed=0)
    ref, _ = plan.tem_run(*f)
    ref = ref.cpu().numpy()
    plan.close()
    for i, n in enumerate(_lib.RESULT_NAMES):
        got = np.load(str(tmp_path / "d1" / (n + ".npy")))
        assert got.dtype == np.float64 and got.shape == ref[i].shape, (n, got.dtype, got.shape)
        assert np.max(np.abs(got - ref[i])) <= 1e-12 * np.max(np.abs(ref[i])), n
    _run(SMALL + ["--dump-outputs", str(tmp_path / "d2")])
    for n in NAMES:
        assert np.array_equal(np.load(str(tmp_path / "d1" / (n + ".npy"))), np.load(str(tmp_path / "d2" / (n + ".npy")))), n


@pytest.mark.gpu
def test_full_run_keeps_the_extras():
    """--full: the CPU baseline with the parity check on the timed path, and the --also shapes beside the metric."""
    rec = _run(SMALL + ["--full", "--also", "ne8x12x2"])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0
    assert rec["cpu_baseline"]["value"] > 0 and rec["parity_vs_oracle_on_sample"]["ok"], rec.get("parity_vs_oracle_on_sample")
    assert rec["other_workloads"]["ne8x12x2"]["ms_per_step"] > 0
