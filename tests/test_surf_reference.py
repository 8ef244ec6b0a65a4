"""The CPU oracle's SURF descriptor against tests/surf_ref.py (plain numpy, written from the Java) on non-default sample grids.

test_oracle_known_answers.py pins the oracle's descriptor at ConfigSurfDescribe's defaults only; tests/test_gpu_surf_configs.py compares
the HIP kernels with the oracle on every geometry below, so the oracle is pinned here first.

Tolerance, derived: both sides form the same fp32 gradients and add them up in fp64 in the same order, from weights built by the same
expressions with the same libm.  A sum of n fp64 terms taken in another order would differ by at most about n * 2^-53 of the sum of
magnitudes; the largest grid has n = 44^2 = 1936 samples, 1936 * 2^-53 = 2.1e-13, so 1e-12 absolute on the unit-norm descriptor would
leave a margin of more than four.  The two implementations turn out bit-identical, so that is what is asserted.

Fast grids with an odd widthLargeGrid * widthSubRegion -- (3, 5) -- are a refusal, not a geometry: DescribePointSurf's constructor builds
its weight kernel 2 * (regionSize / 2) wide and features() then throws "Weighting kernel has an unexpected size"
(DescribePointSurf.java:122-123, 241-243).  Both implementations raise.  (2, 5) and (6, 5) take its place as the fast grids of five-wide
sub-regions and another dof.
"""
import math

import numpy as np
import pytest

import surf_ref

# (stable, SurfCfg fields): the geometry table of tests/test_gpu_surf_configs.py
STABLE = [
    dict(widthLargeGrid=3, widthSubRegion=5, overLap=2),
    dict(widthLargeGrid=4, widthSubRegion=7, overLap=1),
    dict(widthLargeGrid=4, widthSubRegion=6, overLap=3),
    dict(widthLargeGrid=2, widthSubRegion=12, overLap=2),
    dict(widthLargeGrid=6, widthSubRegion=5, overLap=2),
    dict(widthLargeGrid=8, widthSubRegion=5, overLap=2),
    dict(widthSample=5, sigmaLargeGrid=1.0, sigmaSubRegion=4.0),
]
FAST = [
    dict(widthLargeGrid=2, widthSubRegion=5),
    dict(widthLargeGrid=6, widthSubRegion=5),
    dict(widthLargeGrid=4, widthSubRegion=3),
    dict(widthLargeGrid=2, widthSubRegion=8, weightSigma=2.0),
    dict(widthLargeGrid=2, widthSubRegion=16),
    dict(widthLargeGrid=1, widthSubRegion=4),
    dict(widthSample=2, weightSigma=2.0),
]
GEOMETRIES = [(True, g) for g in STABLE] + [(False, g) for g in FAST]

# x, y, angle, scale: interior, fractional, rotated, the three scales, and grids that leave the 80x70 image at each border and corner
POINTS = [
    (40, 35, 0.0, 1.0), (40.3, 34.7, 0.75, 1.0), (40, 35, math.pi / 2, 1.5), (37.6, 33.2, -2.3, 1.5), (40, 35, 0.75, 4.7),
    (40.5, 35.5, -2.3, 4.7), (2, 35, 0.0, 1.0), (77.5, 35, 0.75, 1.0), (40, 1.5, math.pi / 2, 1.0), (40, 68, -2.3, 1.5),
    (0, 0, 0.0, 1.0), (79, 69, 0.75, 1.5),
]


def _id(p):
    stable, g = p
    return ("stable-" if stable else "fast-") + "-".join("%s" % v for v in g.values())


@pytest.fixture(scope="module")
def ii80(orc):
    return orc.integral(orc.noise_image(80, 70, 11))


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_id)
def test_oracle_descriptor_equals_numpy_reference(orc, ii80, geometry):
    stable, g = geometry
    cfg = orc.SurfCfg(**g)
    a = ii80.array()
    dof = cfg.widthLargeGrid ** 2 * 4
    inside = 0
    for (x, y, angle, scale) in POINTS:
        for normalize in (True, False):
            got, _ = orc.describe(ii80, x, y, angle, scale, stable, cfg, normalize)
            want = surf_ref.describe(a, x, y, angle, scale, stable, cfg.widthLargeGrid, cfg.widthSubRegion, cfg.widthSample, cfg.weightSigma,
                                     cfg.overLap, cfg.sigmaLargeGrid, cfg.sigmaSubRegion, normalize)
            assert got.shape == want.shape == (dof,)
            assert np.array_equal(got, want), (x, y, angle, scale, normalize, float(np.max(np.abs(got - want))))
            assert np.all(np.isfinite(got))
            if normalize and np.any(got):
                assert abs(np.linalg.norm(got) - 1) < 1e-12
        radius = (cfg.widthLargeGrid * cfg.widthSubRegion) // 2 + (cfg.overLap if stable else 0)
        inside += surf_ref.sample_boxes_inside(a.shape, x, y, math.cos(angle), math.sin(angle), scale, radius, cfg.widthSample)
    # the point list reaches both gradient forms on every geometry
    assert 0 < inside < len(POINTS)


def test_fast_grid_of_odd_width_is_refused_by_both(orc, ii80):
    cfg = orc.SurfCfg(widthLargeGrid=3, widthSubRegion=5)
    with pytest.raises(ValueError, match="unexpected size"):
        orc.describe(ii80, 40, 35, 0.0, 1.0, False, cfg)
    with pytest.raises(ValueError, match="unexpected size"):
        surf_ref.describe(ii80.array(), 40, 35, 0.0, 1.0, False, 3, 5)
    with pytest.raises(ValueError, match="unexpected size"):
        orc.Surf(False, sd=cfg)
    # the stable descriptor never reads that kernel (DescribePointSurfMod.features :121-192): an odd grid is fine
    f, _ = orc.describe(ii80, 40, 35, 0.0, 1.0, True, cfg)
    assert abs(np.linalg.norm(f) - 1) < 1e-12 and orc.Surf(True, sd=cfg).dof == 36


# ---------------------------------------------------------------------------------------------------
# FT:alg/feature/describe/BaseTestDescribeSurf.java:139-212 on non-default grids, per sub-region over dof/4 groups.  The reference's 50x60
# image holds the default grid only; 100x110 holds the widest grid here (44 samples) at scale 1.5.
# ---------------------------------------------------------------------------------------------------
ANALYTIC = [(True, dict(widthLargeGrid=3, widthSubRegion=5, overLap=2)), (True, dict(widthLargeGrid=6, widthSubRegion=5, overLap=2)),
            (True, dict(widthLargeGrid=4, widthSubRegion=7, overLap=1)), (True, dict(widthLargeGrid=8, widthSubRegion=5, overLap=2)),
            (False, dict(widthLargeGrid=2, widthSubRegion=8, weightSigma=2.0)), (False, dict(widthLargeGrid=6, widthSubRegion=5)),
            (False, dict(widthLargeGrid=4, widthSubRegion=3)), (False, dict(widthLargeGrid=1, widthSubRegion=4))]


@pytest.mark.parametrize("geometry", ANALYTIC, ids=_id)
def test_descriptor_analytic_on_other_grids(orc, geometry):
    stable, g = geometry
    cfg = orc.SurfCfg(**g)
    dof = cfg.widthLargeGrid ** 2 * 4
    w, h = 100, 110

    def both(ii, x, y, angle, scale):
        f, _ = orc.describe(ii, x, y, angle, scale, stable, cfg)
        r = surf_ref.describe(ii.array(), x, y, angle, scale, stable, cfg.widthLargeGrid, cfg.widthSubRegion, cfg.widthSample, cfg.weightSigma,
                              cfg.overLap, cfg.sigmaLargeGrid, cfg.sigmaSubRegion)
        assert f.shape == r.shape == (dof,)
        return f, r

    ii = orc.integral(orc.Gray.from_array(np.full((h, w), 50, np.float32)))
    for f in both(ii, 40, 40, 0.75, 1):       # features_constant
        assert np.all(np.abs(f) < 1e-4)
    yy, xx = np.mgrid[0:h, 0:w]
    ii = orc.integral(orc.Gray.from_array((1.0 * xx + 0.0 * yy).astype(np.float32)))   # TestImplSurfDescribeOps.createGradient(0, input)
    for f in both(ii, 45, 45, 0.0, 1):        # features_increasing, along x
        for i in range(0, dof, 4):
            assert abs(f[i] - f[i + 1]) < 1e-4 and f[i] > 0 and abs(f[i + 2]) < 1e-4 and abs(f[i + 3]) < 1e-4
    for f in both(ii, 45, 45, math.pi / 2, 1):   # along y
        for i in range(0, dof, 4):
            assert abs(-f[i + 2] - f[i + 3]) < 1e-4 and f[i + 2] < 0 and abs(f[i]) < 1e-4 and abs(f[i + 1]) < 1e-4
    for f in both(ii, 50, 50, 0.0, 1.5):      # features_fraction
        for i in range(0, dof, 4):
            assert abs(f[i] - f[i + 1]) < 1e-4 and f[i] > 0 and abs(f[i + 2]) < 1e-4 and abs(f[i + 3]) < 1e-4
        assert abs(np.linalg.norm(f) - 1) < 1e-12


# ---------------------------------------------------------------------------------------------------
# FT:alg/feature/describe/impl/TestImplSurfDescribeOps.java:47-75 (gradientInner == naiveGradient, 1e-4) for sample widths 2, 3 and 5:
# the no-border gradient, the bounds-checked gradient and the oracle's agree on a 5x5 sample region at every scale of the reference's
# sweep, and none of them is zero.  The reference fills the integral image itself with noise; so does this.
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("widthSample", [2, 3, 5])
def test_noborder_gradient_equals_checked_gradient(orc, widthSample):
    import ctypes as C
    L = orc.lib()
    ii = orc.JavaRandom(234).fillUniform(orc.Gray(80, 100), 0, 100)
    a = ii.array()
    radii = set()
    for k in range(1, 10):
        scale = 0.2 * k
        r = surf_ref.grad_radius(widthSample * scale)
        radii.add(r)
        for y in range(5):
            for x in range(5):
                px, py = int(8 + 0.5 + x * scale), int(9 + 0.5 + y * scale)
                nb = surf_ref.gradient_noborder(a, r, px, py)
                ck = surf_ref.gradient_checked(a, r, px, py)
                gx, gy = C.c_float(0), C.c_float(0)
                assert L.orc_sparse_gradient(ii.c(), widthSample * scale, px, py, C.byref(gx), C.byref(gy)) == 1
                assert abs(float(nb[0]) - float(ck[0])) <= 1e-4 and abs(float(nb[1]) - float(ck[1])) <= 1e-4
                assert abs(float(nb[0]) - gx.value) <= 1e-4 and abs(float(nb[1]) - gy.value) <= 1e-4
                assert nb[0] != 0 and nb[1] != 0
    assert len(radii) >= 2    # the sweep changes the kernel radius


@pytest.mark.parametrize("widthSample", [2, 3, 5])
def test_gradient_is_the_box_difference_of_the_pixels_and_zero_outside(orc, widthSample):
    """On integer pixels whose sums stay below 2^24 the fp32 integral image is exact, so the twelve-tap gradient equals the difference of
    the two pixel boxes exactly.  Outside isInBounds the checked form returns (0, 0) and the no-border form is never asked."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 101, (40, 36)).astype(np.float32)
    a = orc.integral(orc.Gray.from_array(img)).array()
    for scale in (1.0, 1.5, 4.7):
        r = surf_ref.grad_radius(widthSample * scale)
        for y in range(-2, 42, 3):
            for x in range(-2, 38, 3):
                inb = surf_ref.gradient_in_bounds(a.shape, r, x, y)
                assert inb == (x - r - 1 >= 0 and y - r - 1 >= 0 and x + r <= 35 and y + r <= 39)
                gx, gy = surf_ref.gradient_checked(a, r, x, y)
                if inb:
                    nx, ny = surf_ref.gradient_naive(img, r, x, y)
                    assert abs(float(gx) - nx) <= 1e-4 and abs(float(gy) - ny) <= 1e-4
                else:
                    assert gx == 0 and gy == 0
                    with pytest.raises(IndexError):
                        surf_ref.gradient_noborder(a, r, x, y)
