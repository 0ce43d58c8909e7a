"""Two real processes on one GPU: the product sharding drivers (pytemdiags_amd/sharding.py) with the
HIP engine as backend and torch.distributed collectives between the ranks (gloo backend, which
all-reduces device tensors; both ranks share cuda:0 -- RCCL itself needs one GPU per rank).
Checks ncol sharding (mirror-symmetric shards, 5 all-reduces incl. the tracer) and time sharding
(no data-path collective, ragged gather) against the unsharded run on the same inputs."""
import os
import socket
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NE, NLEV, NT = 8, 12, 5          # D = 60: four d-tiles, the smallest shape the one-pass forms take
REPLAN_NT = (NT, 7, 1, NT)       # the shapes of the "ncol-replan" mode, one runner.set_tem each (D = 60, 84, 12, 60)
REPLAN_NT_MAX = 7


def _inputs(nt=NT):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(NE)
    plev = synth.pressure_levels(NLEV)
    f = synth.analytic_fields(lat, lon, plev, nt, seed=21)
    q = synth.analytic_tracer(lat, lon, plev, nt)
    lat_zm = (np.arange(-90, 91, 1.0)[1:] + np.arange(-90, 91, 1.0)[:-1]) / 2
    return lat, plev, f, q, lat_zm


def _worker(rank, world, port, mode, ret):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from pytemdiags_amd import engine, sharding
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lat, plev, f, q, lat_zm = _inputs(REPLAN_NT_MAX if mode == "ncol-replan" else NT)
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")   # noqa: E731
        if mode in ("ncol", "ncol-sliced"):
            mine = sharding.symmetric_ncol_shards(lat, world)[rank]
            # "ncol-sliced": the plans run the single sweep (forced: this grid is below the automatic threshold), the
            # tail is time sliced -- all-reduce of the pre-pass sums, reduce-scatter of the projections, this rank
            # finishes its own snapshots; the assembled time axis must be the unsharded run
            plan = engine.Plan(lat[mine], lat_zm, 50, defer_finalize=True,
                               form="single-sweep" if mode == "ncol-sliced" else None)
            runner = sharding.NcolShardedTEM(plan, tail="sliced" if mode == "ncol-sliced" else "replicated")
            if mode == "ncol-sliced":
                runner.set_tem(NLEV, NT, plev * 100)
                assert runner.sliced and runner.my_snapshots() == sharding.shard_bounds(NT, world, rank)
            else:
                plan.set_tem(NLEV, NT, plev * 100)
            loc = [dev(x[mine]) for x in f]
            res, _ = runner.run(*loc)
            tres, _ = runner.run_tracer(dev(q[mine]), loc[1], loc[3])
            if mode == "ncol-sliced":
                assert res.shape[-1] == runner.my_snapshots()[1] - runner.my_snapshots()[0]
                res, tres = sharding.gather_time(res), sharding.gather_time(tres)
            out = torch.cat([res, tres])
            paired = plan.paired
        elif mode == "ncol-replan":
            # one plan per rank through a sequence of shapes and runners: [NT] sliced; [7] sliced again (the
            # plan-build collectives a second time); [1] nt < world, so every rank leaves the single sweep for the
            # replicated tail; [NT] back to the sliced tail; then a second runner on the same plan
            mine = sharding.symmetric_ncol_shards(lat, world)[rank]
            plan = engine.Plan(lat[mine], lat_zm, 50, defer_finalize=True, form="single-sweep")
            runner = sharding.NcolShardedTEM(plan)
            own_G = plan.matrix(sharding.MAT_GRAM).clone()
            own_Gx, outs = None, []
            for step, nt in enumerate(REPLAN_NT + (6,)):
                if step == len(REPLAN_NT):
                    runner = sharding.NcolShardedTEM(plan, tail="sliced")
                    assert torch.equal(plan.matrix(sharding.MAT_GRAM), own_G)
                runner.set_tem(NLEV, nt, plev * 100)
                assert runner.sliced == (nt >= world), (nt, runner.sliced)
                if runner.sliced:
                    if own_Gx is None:
                        own_Gx = plan.matrix(sharding.MAT_GX).clone()
                    assert torch.equal(plan.matrix(sharding.MAT_GX), own_Gx)      # not the all-reduced matrix
                res, _ = runner.run(*[dev(x[mine][:, :, :nt]) for x in f])
                if runner.sliced:
                    res = sharding.gather_time(res)
                assert res.shape[-1] == nt
                outs.append(res)
            # backend.set_tem behind the runner's back: the time axis must be cut for the new shape at the next step
            plan.set_tem(NLEV, REPLAN_NT_MAX, plev * 100)
            res, _ = runner.run(*[dev(x[mine][:, :, :REPLAN_NT_MAX]) for x in f])
            assert runner.my_snapshots() == sharding.shard_bounds(REPLAN_NT_MAX, world, rank)
            outs.append(sharding.gather_time(res))
            out = torch.cat(outs, dim=-1)
            paired = plan.paired
        else:
            plan = engine.Plan(lat, lat_zm, 50)
            runner = sharding.TimeShardedTEM(plan, NT)
            t0, t1 = runner.t0, runner.t1
            plan.set_tem(NLEV, t1 - t0, plev * 100)
            res, _ = runner.run(*[dev(x[:, :, t0:t1]) for x in f])
            out = sharding.gather_time(res)
            paired = plan.paired
        bad = plan.status()
        plan.close()
        if rank == 0:
            ret.put((out.cpu().numpy(), bool(paired), bool(bad)))
    finally:
        dist.destroy_process_group()


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("mode", ["ncol", "ncol-sliced", "time"])
def test_two_ranks_on_one_gpu(mode):
    import torch.multiprocessing as mp
    if mode == "ncol-sliced" and (any(os.environ.get(k) == "1" for k in ("TEMX_NO_SYM", "TEMX_NO_CLS", "TEMX_TWO_PASS", "TEMX_NO_QR"))
                                  or os.environ.get("TEMX_SINGLE_SWEEP") == "0"):
        pytest.skip("the environment forces another form of the sweeps: no single sweep, no time-sliced tail")
    from pytemdiags_amd import engine
    lat, plev, f, q, lat_zm = _inputs()
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, mode, ret)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got, paired, bad = ret.get(timeout=300)
    finally:      # a crashed rank must not leave its sibling running (and holding the GPU)
        for p in procs:
            p.join(timeout=120)
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)
    assert [p.exitcode for p in procs] == [0, 0]
    assert paired == (os.environ.get("TEMX_NO_SYM") != "1") and not bad
    # unsharded reference run in this process
    plan = engine.Plan(lat, lat_zm, 50)
    plan.set_tem(NLEV, NT, plev * 100)
    d = [torch.as_tensor(x, device="cuda:0") for x in f]
    ref, _ = plan.tem_run(*d)
    ref = ref.cpu().numpy()
    if mode.startswith("ncol"):
        tref, _ = plan.tracer_run(torch.as_tensor(q, device="cuda:0"), d[1], d[3])
        ref = np.concatenate([ref, tref.cpu().numpy()])
    plan.close()
    assert got.shape == ref.shape
    for i in range(ref.shape[0]):
        err = np.max(np.abs(got[i] - ref[i])) / np.max(np.abs(ref[i]))
        assert err <= 1e-11, (mode, i, err)


def test_bench_line_at_two_ranks_and_failure_exit_code():
    """`bench.py --gpus 2` reports BASELINE configs[3] (one job, ncol-sharded, strong scaling)
    as the metric and configs[2] (time-sharded) beside it; a failing leg ends the run non-zero.  Rehearsed
    with two ranks on this one GPU over gloo (TEMX_BENCH_BACKEND), small shapes."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["TEMX_BENCH_BACKEND"] = "gloo"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--workload", "ne30x72x8", "--time-workload", "ne30x72x9", "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong" and rec["config"]["shard"] == "ncol"
    assert rec["process_group"]["ranks"] == 2 and rec["value"] > 0 and "errors" not in rec
    ow = rec["other_workloads"]
    ts = ow["ne30x72x9:time_sharded"]
    assert ts["scaling"] == "strong" and ts["shard"] == "time" and ts["snapshots_this_rank"] == 4 and ts["value"] > 0      # 9 snapshots in blocks of whole cache lines per row: 4 + 5
    assert ow["ne30x72x8:weak_scaling"]["scaling"] == "weak"
    # a forced failure of the time-sharded leg: the line still comes out, with the error, and the exit code is 4
    env["TEMX_BENCH_FAIL"] = "ne30x72x9:time_sharded"
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode != 0, (p.stdout + p.stderr)[-3000:]
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert "ne30x72x9:time_sharded" in rec["errors"]
    # and of the metric leg itself
    env["TEMX_BENCH_FAIL"] = "main"
    p = subprocess.run(cmd + ["--no-extras"], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode != 0


def test_set_tem_again_on_a_sharded_runner():
    """runner.set_tem with a new nt (once with nt < world: the sliced decision flips, and flips back), a second
    NcolShardedTEM on the same plan and a backend.set_tem between two steps: every run is the unsharded run on the
    same fields.  The matrices a rank contributes to the plan-build all-reduces (TEMX_MAT_GRAM, TEMX_MAT_GX) must
    stay its own, or the second all-reduce installs world x the job's matrix.  One time limit for the two children,
    no second attempt."""
    import torch.multiprocessing as mp
    if any(os.environ.get(k) == "1" for k in ("TEMX_NO_SYM", "TEMX_NO_CLS", "TEMX_TWO_PASS", "TEMX_NO_QR")) or \
            os.environ.get("TEMX_SINGLE_SWEEP") == "0":
        pytest.skip("the environment forces another form of the sweeps: no single sweep, no time-sliced tail")
    from pytemdiags_amd import engine
    import queue
    import time
    lat, plev, f, q, lat_zm = _inputs(REPLAN_NT_MAX)
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, "ncol-replan", ret)) for r in range(2)]
    for p in procs:
        p.start()
    got = None
    try:
        deadline = time.monotonic() + 300
        while got is None and time.monotonic() < deadline:
            try:
                got, paired, bad = ret.get(timeout=2)
            except queue.Empty:       # (a child that failed an assertion has nothing to send: do not wait it out)
                if any(p.exitcode not in (None, 0) for p in procs):
                    break
    finally:
        for p in procs:
            p.join(timeout=120)
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=30)
    assert [p.exitcode for p in procs] == [0, 0] and got is not None
    assert not bad
    plan = engine.Plan(lat, lat_zm, 50)
    refs = []
    for nt in REPLAN_NT + (6, REPLAN_NT_MAX):
        plan.set_tem(NLEV, nt, plev * 100)
        r, _ = plan.tem_run(*[torch.as_tensor(np.ascontiguousarray(x[:, :, :nt]), device="cuda:0") for x in f])
        refs.append(r.cpu().numpy())
    plan.close()
    ref = np.concatenate(refs, axis=-1)
    assert got.shape == ref.shape
    t0 = 0
    for step, r in enumerate(refs):
        t1 = t0 + r.shape[-1]
        for i in range(r.shape[0]):
            err = np.max(np.abs(got[i][..., t0:t1] - r[i])) / np.max(np.abs(r[i]))
            assert err <= 1e-11, (step, r.shape[-1], i, err)
        t0 = t1
