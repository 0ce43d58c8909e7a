"""The inputs of tests/test_gpu_regimes.py, part B, checked without a GPU: on synth.jet_fields the oracle must agree
with ITSELF far inside the 1e-10 it is used at, or a miss there says nothing about the engine.  Its two constructions
of the basis (scipy's sph_harm and the three-term recurrence) are each good to a few ulp; what they differ by in the
results is the conditioning of the reference's formulae on these fields.  With eddies whose flux means all but vanish
(waves in quadrature or of different wavenumber: the first version of the generator) they differed by 6e-11 at
eps = 0.1 and 3.4e-10 at eps = 0.01; held to a fifth of 1e-10 here."""
import numpy as np
import pytest

from conftest import fieldnorm_err


@pytest.mark.parametrize("width", [8.0, 4.0, 2.0])
def test_oracle_is_reproducible_on_jet_fields(width):
    from oracle import tem_oracle as orc
    from pytemdiags_amd import _lib, synth
    lat, lon = synth.cubed_sphere_gll(12)
    nlev, nt = 16, 4
    plev = synth.pressure_levels(nlev)
    for eps in (1.0, 0.1, 0.01):
        f = synth.jet_fields(lat, lon, plev, nt, width=width, eps=eps, seed=1)
        a = orc.TEMOracle(*f, lat, plev, L=50, mode="factorised")
        b = orc.TEMOracle(*f, lat, plev, L=50, mode="factorised", basis="recurrence")
        errs = {n: fieldnorm_err(getattr(b, n)(), getattr(a, n)()) for n in _lib.RESULT_NAMES}
        errs.update({n: fieldnorm_err(getattr(b, n), getattr(a, n)) for n in _lib.ZONAL_NAMES})
        worst = max(errs, key=errs.get)
        print("width %g eps %g: the oracle's two bases differ by %.1e in %s" % (width, eps, errs[worst], worst))
        assert errs[worst] <= 2e-11, (width, eps, worst, errs[worst])
        # and the fluxes are of the size of the products they are means of (not a small remainder of them)
        for flux, pa, pb in (("upvpb", "up", "vp"), ("upwappb", "up", "wapp"), ("vptpb", "vp", "thetap")):
            scale = float(np.max(np.abs(getattr(a, pa))) * np.max(np.abs(getattr(a, pb))))
            assert float(np.max(np.abs(getattr(a, flux)))) >= 1e-2 * scale, (width, eps, flux)
