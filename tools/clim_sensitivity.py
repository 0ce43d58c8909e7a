#!/usr/bin/env python3
"""How far one unit in the last place of the time-mean fields moves the stationary set of the numpy oracle: the
figures ``ORACLE_SHIFT_PER_ULP`` of tests/test_gpu_clim.py.  CPU only, a few seconds.

For each grid of that test (cs4, cs8, the 3000 random latitudes; 6 levels, nt = 5, L = 20, seed 5) the time-mean fields
are multiplied by ``1 + 2^-53 s`` with ``s`` drawn from {-1, 0, 1} per point, three draws, and the oracle's stationary
TEM (``TEMOracle`` of the time-mean fields) is compared with the unperturbed one: max |delta| / max |quantity| over the
ten results and sixteen zonal intermediates, the worst quantity and draw reported.

  python tools/clim_sensitivity.py
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from oracle import tem_oracle as orc  # noqa: E402
from pytemdiags_amd import _lib, synth  # noqa: E402


def grid(kind):
    if kind == "random":
        rng = np.random.default_rng(3)
        return np.rad2deg(np.arcsin(rng.uniform(-1, 1, 3000))), rng.uniform(0, 360, 3000)
    return synth.cubed_sphere_gll(int(kind[2:]))[:2]


def quantities(o):
    out = {n: getattr(o, n)() for n in _lib.RESULT_NAMES}
    out.update({n: getattr(o, n) for n in _lib.ZONAL_NAMES})
    return out


def main():
    for kind in ("cs4", "cs8", "random"):
        lat, lon = grid(kind)
        plev = synth.pressure_levels(6)
        mean = [x.mean(axis=2, keepdims=True) for x in synth.analytic_fields(lat, lon, plev, 5, seed=5)]
        base = quantities(orc.TEMOracle(*mean, lat, plev, L=20, mode="factorised"))
        rng = np.random.default_rng(0)
        worst = (0.0, "")
        for _ in range(3):
            moved = [x * (1 + 2.0 ** -53 * rng.choice([-1.0, 0.0, 1.0], x.shape)) for x in mean]
            q = quantities(orc.TEMOracle(*moved, lat, plev, L=20, mode="factorised"))
            for n, x in base.items():
                worst = max(worst, (float(np.abs(q[n] - x).max() / np.abs(x).max()), n))
        print("%-6s shift per unit in the last place %.2e (%s)" % (kind, worst[0], worst[1]))


if __name__ == "__main__":
    main()
