"""The single sweep of fp64 fields hands the class sums of a class-group from the waves that read to the waves that
project through two counters in LDS (csrc/kernels_op2.hpp, sweep_osr_kernel<SYNC = 1>, the default) or through two
workgroup barriers (TEMX_OPT_OS_SYNC = 1).  Same sums, same MFMAs, same order per accumulator: every output of the
flag form must equal the barrier form's bit for bit, and no wave may have given up waiting (temx_status)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


def _lat_zm():
    e = np.arange(-90, 91, 1.0)
    return (e[1:] + e[:-1]) / 2


def _pair(lat, L, monkeypatch):
    """Two plans on the single-sweep form: hand-over by flags (the default) and by barriers."""
    from pytemdiags_amd import _lib, engine
    for k in ("TEMX_OS_SYNC", "TEMX_OS_MAP", "TEMX_SINGLE_SWEEP", "TEMX_TWO_PASS", "TEMX_NO_CLS", "TEMX_NO_SYM", "TEMX_NO_QR"):
        monkeypatch.delenv(k, raising=False)
    flags = engine.Plan(lat, _lat_zm(), L, form="single-sweep")
    barrier = engine.Plan(lat, _lat_zm(), L, form="single-sweep")
    barrier.configure(os_sync="barrier")
    return _lib, flags, barrier


def _check_pair(_lib, flags, barrier, nlev, nt, plev, f, qs, W):
    for p in (flags, barrier):
        p.set_tem(nlev, nt, plev * 100)
        assert p.single_sweep and p.option(_lib.OPT_FORM) == _lib.FORM_SINGLE_SWEEP
    assert flags.option(_lib.OPT_OS_SYNC) == 0 and barrier.option(_lib.OPT_OS_SYNC) == 1
    d = [_dev(x) for x in f]
    dq = [_dev(q) for q in qs]
    out = []
    for p in (flags, barrier):
        o = {}
        o["res"], o["zon"] = p.tem_run(*d, want_zonal=True)
        assert not p.status()
        for n in (1, 2):                                   # the one-tracer and the two-tracer kind of the sweep
            for i, (tr, tz) in enumerate(p.tracers_run(dq[:n], d[1], d[3], want_zonal=True)):
                o["tres%d%d" % (n, i)], o["tzon%d%d" % (n, i)] = tr, tz
            assert not p.status()
        o["As"] = p.tem_os_prepass(*d)                     # the pre-pass: the same kernel on a subsample of the groups
        assert not p.status()
        o["proj"] = p.tem_os_sweep(*d, o["As"])
        assert not p.status()
        o["projW"] = p.tem_os_sweep(*d, o["As"], nslices=W)
        assert not p.status()
        out.append(o)
    a, b = out
    assert a.keys() == b.keys()
    for k in a:
        assert torch.isfinite(a[k]).all(), k
        assert torch.equal(a[k], b[k]), k
    for p in (flags, barrier):
        p.close()


@pytest.mark.parametrize("ne,nlev,nt,L,W", [
    (16, 10, 7, 50, 3),       # D = 70: one full window of 64 columns and a masked one; 7 + 13 blocks
    (30, 9, 7, 50, 2),        # D = 63: a single masked window
    (10, 11, 7, 28, 3),       # D = 77, 4 + 8 blocks
    (8, 10, 5, 12, 2),        # D = 50, 2 + 4 blocks (the single sweep needs four d-tiles of 16 columns: D >= 49)
])
def test_flag_form_equals_barrier_form_on_cubed_spheres(ne, nlev, nt, L, W, monkeypatch):
    from pytemdiags_amd import synth
    lat, lon = synth.cubed_sphere_gll(ne)
    plev = synth.pressure_levels(nlev)
    f = synth.analytic_fields(lat, lon, plev, nt, seed=23)
    qs = [synth.analytic_tracer(lat, lon, plev, nt, which=k) for k in (0, 1)]
    _lib, flags, barrier = _pair(lat, L, monkeypatch)
    _check_pair(_lib, flags, barrier, nlev, nt, plev, f, qs, W)


def test_flag_form_equals_barrier_form_with_more_work_than_one_round_of_workgroups(monkeypatch):
    """D = 64 x 301 + 10 columns: 302 windows of 64 columns, more workgroups than the GPU has compute units, so that
    workgroups of two rounds overlap; the last window is masked."""
    from pytemdiags_amd import synth
    ne, nlev, nt, L = 6, 46, 419, 28
    assert nlev * nt == 64 * 301 + 10
    lat, lon = synth.cubed_sphere_gll(ne)
    plev = synth.pressure_levels(nlev)
    f = synth.analytic_fields(lat, lon, plev, nt, seed=5)
    qs = [synth.analytic_tracer(lat, lon, plev, nt, which=k) for k in (0, 1)]
    _lib, flags, barrier = _pair(lat, L, monkeypatch)
    _check_pair(_lib, flags, barrier, nlev, nt, plev, f, qs, 4)


def test_flag_form_equals_barrier_form_with_one_batch_and_two_batch_groups(monkeypatch, tmp_path):
    """A lat-lon grid of four longitudes: 40 mirrored pairs of rows (classes of 4 + 4 members: groups of two batches)
    and an equator row (a class of one side and one batch, alone in the last group).  A group shorter than the four
    steps its projection is spread over makes the taker-over flush what is left of the group before; the library's
    own row table (TEMX_DUMP_CROW) is read back to make sure the grid holds both lengths."""
    from pytemdiags_amd import synth
    h, nlon, nlev, nt, L = 40, 4, 9, 7, 12
    north = (np.arange(h) + 0.5) * (90.0 / (h + 0.5))
    rows = np.concatenate([-north[::-1], [0.0], north])
    lat = np.repeat(rows, nlon)
    lon = np.tile(np.arange(nlon) * (360.0 / nlon), rows.size)
    plev = synth.pressure_levels(nlev)
    f = synth.analytic_fields(lat, lon, plev, nt, seed=3)
    qs = [synth.analytic_tracer(lat, lon, plev, nt, which=k) for k in (0, 1)]
    dump = tmp_path / "crow.bin"
    monkeypatch.setenv("TEMX_DUMP_CROW", str(dump))        # (written when a plan builds its latitude classes)
    _lib, flags, barrier = _pair(lat, L, monkeypatch)
    monkeypatch.delenv("TEMX_DUMP_CROW")
    raw = np.fromfile(dump, dtype=np.int32)
    ngroups = int(raw[0])
    lengths = np.diff(raw[2:2 + ngroups + 1])
    print("batches per class-group:", np.unique(lengths, return_counts=True))
    assert 1 in lengths and 2 in lengths
    _check_pair(_lib, flags, barrier, nlev, nt, plev, f, qs, 2)
