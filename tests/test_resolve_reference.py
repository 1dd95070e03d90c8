"""CPU: the film resolve of the oracle against its float64 statement (tests/resolve_reference.py); the GPU's k_resolve
is held to the same statement in tests/test_gpu_spectral.py.

The assertion (resolve_reference.check): no byte differs from the float64 code by more than one, and a byte differs
by one only where the float64 pre-quantisation value q (in code units) lies within `delta` of a code boundary (the
integers 1 .. 255 for the truncating linear encoding, the half-integers for the rounding sRGB encoding).

Derivation of delta, per byte, with u = 2^-24:
  - s = rgb / w is one correctly rounded division (u).  v = B (A s) is two 3 x 3 products of three rounded
    multiplications and two rounded additions each (3 u each on the sum of the absolute terms).  With one u spare:
    |dv| <= 8 u (|B| |A| |s|).
  - The matrices themselves are float32 in the renderers, built from float32 sums of 471 products: every entry is
    allowed 2 sqrt(471) u = 43 u of its matrix's largest entry (resolve_reference.matrix_allowance: a random-walk
    model of those sums, not a measurement of the code under test; test_oracle_matrices_against_float64 holds the
    oracle's matrices to it): |dv| += |dB| |A| |s| + |B| |dA| |s|.
  - linear: q = 255 v, one more product: delta = 255 |dv| + 2 * 255 u.
  - sRGB: |dv| times 255 times the OETF's steepest slope on [v - |dv|, 1] (12.92 below the knee), plus 255 times the
    error of pbrt's rational polynomial against the exact OETF (`RATIONAL_ERROR`, measured in float64 on two million
    points of [0, 1] and around the knee: a property of the specified approximation), plus 16 u for evaluating it in
    float32 (a square root, two quintic Horner chains, a division, two products, on values <= 1).
By the float64 reference alone, at most 2 % of the bytes that an illuminant's films hold (all sizes, both encodings)
lie within delta of a boundary: the test cannot pass by excusing everything.  Per film the share is 0-1.3 %, except
illuminant A in the sRGB encoding with 2.0-2.4 %: its adaptation triples Z, so more of the steep foot of the OETF is
reached with large |s|."""
import numpy as np
import pytest

import resolve_reference as rr
from computational_ray_tracer_amd import capi


def test_published_bradford_pair_is_an_inverse_pair():
    assert np.abs(rr.XYZ_FROM_LMS @ rr.LMS_FROM_XYZ - np.eye(3)).max() < 1e-6


def test_matrices_second_derivation():
    """D65 adapts to itself; every adaptation maps the illuminant's white (Y = 1) onto D65's; RGBFromXYZ maps the
    white to (1, 1, 1) and each primary's chromaticity onto its own axis; the published chromaticities."""
    x, y = rr.chromaticity(capi.RT_ILLUM_D65)
    assert abs(x - 0.31272) < 2e-5 and abs(y - 0.32903) < 2e-5
    xa, ya = rr.chromaticity(capi.RT_ILLUM_A)
    assert abs(xa - 0.4476) < 1e-3 and abs(ya - 0.4074) < 1e-3
    white = rr._from_xy(x, y)
    for illum in rr.ILLUMS:
        a, b = rr.matrices(illum)
        src = rr._from_xy(*rr.chromaticity(illum))
        assert np.allclose(a @ src, white, atol=2e-6)
        assert np.allclose(b @ white, 1.0, atol=1e-12)
        for k, (px, py) in enumerate(rr.PRIMARIES):
            rgb = b @ rr._from_xy(px, py)
            assert rgb[k] > 0 and np.allclose(np.delete(rgb, k), 0.0, atol=1e-12)
        assert (illum == capi.RT_ILLUM_D65) == np.allclose(a, np.eye(3), atol=2e-6)
    # the sRGB matrix as published (IEC 61966-2-1), to its four digits
    assert np.allclose(rr.matrices(capi.RT_ILLUM_D65)[1], [[3.2406, -1.5372, -0.4986], [-0.9689, 1.8758, 0.0415],
                                                            [0.0557, -0.2040, 1.0570]], atol=6e-4)


def test_encodings():
    assert rr.oetf_exact(0.0) == 0 and rr.oetf_exact(1.0) == pytest.approx(1.0, abs=1e-15)
    assert rr.oetf_exact(0.5) == pytest.approx(0.7353569830524495, abs=1e-12)          # 1.055 * 0.5^(1/2.4) - 0.055
    assert rr.oetf_exact(0.002) == pytest.approx(0.02584, abs=1e-15)
    assert 0 < rr.RATIONAL_ERROR < 1e-5, rr.RATIONAL_ERROR          # far below half a code (2e-3)
    film = np.array([[0.5, 0.5, 0.5, 1.0], [2.0, -1.0, 254.9999 / 255, 1.0]], np.float32)
    xyz_from_rgb = np.linalg.inv(rr.matrices(capi.RT_ILLUM_D65)[1])
    film[:, :3] = film[:, :3] @ xyz_from_rgb.T.astype(np.float32)                 # the XYZ of these linear rgb
    e = rr.expected(film, capi.RT_ILLUM_D65, srgb=False)
    assert list(e["code"][0]) == [127, 127, 127] and list(e["code"][1][:2]) == [255, 0]
    e = rr.expected(film, capi.RT_ILLUM_D65, srgb=True)
    assert list(e["code"][0]) == [188, 188, 188] and list(e["code"][1][:2]) == [255, 0]


@pytest.mark.parametrize("illum", rr.ILLUMS)
def test_inputs_are_mostly_away_from_the_boundaries(illum):
    """By the float64 reference alone: at most 2 % of the bytes examined under an illuminant lie within delta of a
    code boundary."""
    near, total = 0, 0
    for n in rr.SIZES:
        film = rr.synthetic_film(n, illum)
        for srgb in (False, True):
            e = rr.expected(film, illum, srgb)
            m = e["distance"] <= e["delta"]
            print(n, illum, srgb, "near", m.mean(), "median delta", np.median(e["delta"]), "max", e["delta"].max())
            near, total = near + m.sum(), total + m.size
    assert near <= 0.02 * total, near / total


@pytest.mark.parametrize("illum", rr.ILLUMS)
@pytest.mark.parametrize("n", rr.SIZES)
def test_inputs_hold_the_edge_rows(n, illum):
    """Pixels without weight expect 0; the knee rows straddle the knee; the values span [-0.1, 1.2]."""
    film = rr.synthetic_film(n, illum)
    assert film.shape == (n, 4) and film.dtype == np.float32
    e = rr.expected(film, illum, True)
    assert set(np.unique(film[e["finite"], 3])) <= {1.0, 256.0}
    if n >= 255:
        assert list(np.flatnonzero(~e["finite"])) == list(range(n - 12, n - 8))
        assert np.all(e["code"][~e["finite"]] == 0)
        a, b = rr.matrices(illum)
        v = film[-8:, :3].astype(np.float64) @ (b @ a).T
        assert np.allclose(v, rr.SRGB_KNEE, rtol=2e-6, atol=0) and (v < rr.SRGB_KNEE).any() and (v > rr.SRGB_KNEE).any()
        u = film[:-12, :3] / film[:-12, 3:4]
        assert u.min() < -0.09 and u.max() > 1.19
    else:
        assert e["finite"].all()


@pytest.mark.parametrize("illum", rr.ILLUMS)
def test_oracle_matrices_against_float64(oracle_lib, illum):
    """The oracle's float32 matrices lie within the allowance that delta grants them."""
    a32, b32 = (np.asarray(m, np.float64).reshape(3, 3).T
                for m in oracle_lib.OracleScene(rr.config(1, illum)).resolve_matrices())
    (a, b), (da, db) = rr.matrices(illum), rr.matrix_allowance(illum)
    print(illum, (np.abs(a32 - a) / da).max(), (np.abs(b32 - b) / db).max())
    assert np.all(np.abs(a32 - a) <= da) and np.all(np.abs(b32 - b) <= db)


@pytest.mark.parametrize("srgb", [False, True])
@pytest.mark.parametrize("illum", rr.ILLUMS)
@pytest.mark.parametrize("n", rr.SIZES)
def test_oracle_resolve_against_float64(oracle_lib, n, illum, srgb):
    film = rr.synthetic_film(n, illum)
    got = oracle_lib.OracleScene(rr.config(n, illum)).resolve(film, srgb)
    off, near = rr.check(got, film, illum, srgb)
    print(n, illum, srgb, "off by one", off, "near a boundary", near)


@pytest.mark.parametrize("srgb", [False, True])
def test_check_can_fail(oracle_lib, srgb):
    """Power: a swapped pair of output channels, the other encoding, a matrix for another illuminant and a single
    byte raised by one code away from a boundary all fail `check`."""
    illum, n = capi.RT_ILLUM_A, 4097
    film = rr.synthetic_film(n, illum)
    good = oracle_lib.OracleScene(rr.config(n, illum)).resolve(film, srgb)
    rr.check(good, film, illum, srgb)
    with pytest.raises(AssertionError):
        rr.check(np.ascontiguousarray(good[:, ::-1]), film, illum, srgb)
    with pytest.raises(AssertionError):
        rr.check(oracle_lib.OracleScene(rr.config(n, illum)).resolve(film, not srgb), film, illum, srgb)
    with pytest.raises(AssertionError):
        rr.check(good, film, capi.RT_ILLUM_D50, srgb)
    e = rr.expected(film, illum, srgb)
    far = np.argwhere((e["distance"] > (0.3 if srgb else 0.4)) & (e["code"] > 0) & (e["code"] < 255))[0]
    one = good.copy()
    one[far[0], far[1]] += 1
    with pytest.raises(AssertionError):
        rr.check(one, film, illum, srgb)
