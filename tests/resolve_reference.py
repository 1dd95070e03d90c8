"""The film resolve (rgb / w -> XYZFromSensorRGB -> sRGB RGBFromXYZ -> 8 bit) in numpy float64, for the XYZ sensor.

Like radiometry_reference.py, on which it builds, this module calls neither the oracle nor the product library; it
reads the committed spectral tables only.  The camera sensors' XYZFromSensorRGB (the reference's transposed
least-squares fit, tests/test_oracle_sensor.py) is left to the existing tests.

  RGBFromXYZ          inverse of the sRGB primaries (0.64, 0.33), (0.30, 0.60), (0.15, 0.06) scaled to the D65 white
                      computed from the table;
  XYZFromSensorRGB    von Kries adaptation in the Bradford cone space from the sensor illuminant's chromaticity
                      (computed from its table) to that white; LMSFromXYZ and XYZFromLMS are the two published
                      matrices of pbrt's WhiteBalance (their product is the identity to 6e-7);
  linear encoding     trunc(255 clamp(v, 0, 1));
  sRGB encoding       round(255 OETF(clamp(v, 0, 1))) with the exact piecewise OETF of IEC 61966-2-1;
  w = 0               0 / 0 is NaN, which encodes as 0; (+-a, +-a, +-a) / 0 with one sign is three equal infinities,
                      which the two products turn into NaN (every row of RGBFromXYZ has entries of both signs and
                      XYZFromSensorRGB a positive diagonal; asserted in `matrices`), so it encodes as 0 as well.

`expected(film, illum, srgb)` returns, per byte, the code, the pre-quantisation value q in code units, the distance
of q from the nearest code boundary and `delta`, the error a float32 evaluation may have (derivation: the docstring
of tests/test_resolve_reference.py).  `check` is the assertion shared by the CPU and GPU tests.
"""
import numpy as np

import radiometry_reference as ref
from computational_ray_tracer_amd import capi, scene

U = 2.0 ** -24                                   # unit roundoff of float32
PRIMARIES = ((0.64, 0.33), (0.30, 0.60), (0.15, 0.06))
LMS_FROM_XYZ = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
XYZ_FROM_LMS = np.array([[0.986993, -0.147054, 0.159963], [0.432305, 0.51836, 0.0492912],
                         [-0.00852866, 0.0400428, 0.968487]])
ILLUMS = (capi.RT_ILLUM_D65, capi.RT_ILLUM_A, capi.RT_ILLUM_D50, capi.RT_ILLUM_F1 + 10)     # D65, A, D50, F11
SIZES = (1, 255, 256, 257, 4097)
SRGB_KNEE = 0.0031308


def _from_xy(x, y):
    return np.array([x / y, 1.0, (1.0 - x - y) / y])


def chromaticity(which):
    """(x, y) of a named illuminant: its table summed against the CIE bars on the integer nanometres."""
    xyz = ref.BARS @ ref.illuminant(which)(ref.LAMBDA)
    return xyz[0] / xyz.sum(), xyz[1] / xyz.sum()


def matrices(illum):
    """(XYZFromSensorRGB, RGBFromXYZ) of the XYZ sensor under `illum`, as (row, column) float64 arrays."""
    white = _from_xy(*chromaticity(capi.RT_ILLUM_D65))
    prim = np.stack([_from_xy(x, y) for x, y in PRIMARIES], axis=1)
    c = np.linalg.solve(prim, white)
    rgb_from_xyz = np.linalg.inv(prim * c[None, :])
    src = _from_xy(*chromaticity(illum))
    corr = (LMS_FROM_XYZ @ white) / (LMS_FROM_XYZ @ src)
    xyz_from_sensor = (XYZ_FROM_LMS * corr[None, :]) @ LMS_FROM_XYZ
    assert np.all(np.diag(xyz_from_sensor) > 0)
    assert np.all(rgb_from_xyz.max(axis=1) > 0) and np.all(rgb_from_xyz.min(axis=1) < 0)
    return xyz_from_sensor, rgb_from_xyz


N_TABLE = 471
MATRIX_REL = 2.0 * np.sqrt(N_TABLE) * U          # 43 u = 2.6e-6


def matrix_allowance(illum):
    """Entrywise |error| allowed to matrices built in float32.  Their entries are ratios and products of a few sums
    of 471 rounded products (the illuminants against the CIE bars).  The rounding errors of such a sum accumulate
    like a random walk, about sqrt(n) u of the sum (the worst case n u = 2.8e-5 is never approached); with a factor
    two for the two or three sums that meet in an entry and for the cofactor inverse (the condition number of
    XYZFromRGB is 4): 2 sqrt(471) u = 43 u of the matrix's largest entry, for every entry."""
    return [np.full((3, 3), MATRIX_REL * np.abs(m).max()) for m in matrices(illum)]


def oetf_exact(v):
    v = np.asarray(v, np.float64)
    return np.where(v <= SRGB_KNEE, 12.92 * v, 1.055 * np.maximum(v, 0.0) ** (1.0 / 2.4) - 0.055)


def oetf_rational(v):
    """pbrt's LinearToSRGB (color.h): 12.92 v up to 0.0031308, above it v p(sqrt v) / q(sqrt v) with two quintics;
    evaluated in float64.  The approximation the renderer is specified to use."""
    v = np.asarray(v, np.float64)
    s = np.sqrt(np.maximum(v, 0.0))
    p = np.polyval([-0.016202083165206348, 0.7551545191665577, 2.0041169284241644, 0.7642611304733891,
                    0.03453868659826638, -0.0016829072605308378], s)
    q = np.polyval([1.0, 1.8970238036421054, 0.6085338522168684, 0.03467195408529984, -0.00004375359692957097,
                    4.178892964897981e-7], s)
    return np.where(v <= SRGB_KNEE, 12.92 * v, p / q * v)


def rational_error(n=2_000_001):
    """max |rational - exact| of the sRGB OETF over a dense grid of [0, 1], in units of the encoded value: a property
    of the specified approximation, not of any implementation."""
    v = np.linspace(0.0, 1.0, n)
    v = np.concatenate([v, SRGB_KNEE * (1 + np.linspace(-1e-3, 1e-3, 2001))])
    return float(np.max(np.abs(oetf_rational(v) - oetf_exact(v))))


RATIONAL_ERROR = rational_error()


def _oetf_slope(v):
    """An upper bound of the OETF's derivative on [v, 1] (it decreases above the knee)."""
    v = np.maximum(np.asarray(v, np.float64), 1e-12)
    return np.minimum(12.92, 1.055 / 2.4 * v ** (1.0 / 2.4 - 1.0))


def expected(film, illum, srgb):
    """dict(code uint8 [n, 3], q, distance, delta float64 [n, 3], finite bool [n]) of a film float32 [n, 4]."""
    film = np.asarray(film, np.float32).astype(np.float64)
    a, b = matrices(illum)
    da, db = matrix_allowance(illum)
    with np.errstate(all="ignore"):
        s = film[:, :3] / film[:, 3:4]
        v = (s @ a.T) @ b.T
    finite = np.all(np.isfinite(s), axis=1)
    assert np.all(np.isnan(v[~finite])), "a pixel without weight must resolve to NaN"
    s0 = np.where(finite[:, None], np.abs(s), 0.0)
    x0 = s0 @ np.abs(a).T
    # |error of v|: 8 u on sum |B| |A| |s| (division 1, each product 3, and 1 spare), and the matrices' entries
    err = 8 * U * (x0 @ np.abs(b).T) + (s0 @ da.T) @ np.abs(b).T + x0 @ db.T
    vc = np.clip(np.where(finite[:, None], v, 0.0), 0.0, 1.0)
    if srgb:
        q = 255.0 * oetf_exact(vc)
        code = np.where(vc >= 1.0, 255.0, np.where(vc <= 0.0, 0.0, np.rint(q)))
        # the error of v through the steepest slope nearby, the rational approximation, and its float32 evaluation
        # (sqrt, two quintic Horner chains of fused multiply-adds, a division and two products: 16 u of a value <= 1)
        delta = 255.0 * (_oetf_slope(vc - err) * err + RATIONAL_ERROR + 16 * U) + 255.0 * U
        boundary = np.clip(np.floor(q), 0.0, 254.0) + 0.5
    else:
        q = 255.0 * vc
        code = np.floor(q)
        delta = 255.0 * err + 255.0 * 2 * U          # and the product 255 v itself
        boundary = np.clip(np.rint(q), 1.0, 255.0)
    code = np.where(finite[:, None], code, 0.0).astype(np.uint8)
    # the code 255 is reached at v = 1 and kept beyond it: the distance from that boundary is taken before the clamp
    far = 255.0 * np.where(finite[:, None], np.maximum(v, 1.0), 1.0) - 255.0
    distance = np.where(finite[:, None], np.abs(q - boundary) + (0.0 if srgb else far), np.inf)
    return dict(code=code, q=q, distance=distance, delta=delta, finite=finite)


def check(got, film, illum, srgb):
    """No byte off by more than one code, and one off only where q lies within delta of a code boundary.  Returns
    (bytes off by one, bytes within delta of a boundary)."""
    e = expected(film, illum, srgb)
    diff = np.abs(np.asarray(got).astype(np.int64) - e["code"].astype(np.int64))
    assert diff.shape == e["code"].shape
    assert diff.max() <= 1, f"a byte differs by {diff.max()} codes"
    near = e["distance"] <= e["delta"]
    bad = (diff == 1) & ~near
    assert not bad.any(), (f"{bad.sum()} bytes are off by one away from a code boundary; the first: q "
                           f"{e['q'][bad][0]!r}, delta {e['delta'][bad][0]:.2e}, got {np.asarray(got)[bad][0]}")
    return int((diff == 1).sum()), int(near.sum())


def synthetic_film(n, illum, seed=7):
    """n pixels: rgb drawn in [-0.1, 1.2] w with w 1 or 256; from 255 pixels on, the last twelve are four without
    weight (0 / 0, and +a / 0, -a / 0, +b / 0 in all three channels) and eight whose linear sRGB value is 0.0031308,
    the knee of the OETF, and 1, 2, 3 float32 steps below and above it."""
    rng = np.random.default_rng(seed + 1000 * n + illum)
    w = np.where(rng.random(n) < 0.5, 1.0, 256.0)
    film = np.concatenate([rng.uniform(-0.1, 1.2, (n, 3)) * w[:, None], w[:, None]], axis=1).astype(np.float32)
    if n >= 255:
        film[-12:-8] = [[0, 0, 0, 0], [0.25, 0.25, 0.25, 0], [-3, -3, -3, 0], [700, 700, 700, 0]]
        a, b = matrices(illum)
        knee = np.float32(SRGB_KNEE)
        for j, steps in enumerate((0, 1, 2, 3, -1, -2, -3, 4)):
            t = knee
            for _ in range(abs(steps)):
                t = np.nextafter(t, np.float32(1 if steps > 0 else 0))
            film[-8 + j, :3] = np.linalg.solve(b @ a, np.full(3, float(t)))
            film[-8 + j, 3] = 1.0
    return film


def frame_linear_srgb(film, illum=capi.RT_ILLUM_D65):
    """The frame mean of film.rgb / film.w through the float64 matrices: linear sRGB."""
    film = np.asarray(film, np.float64)
    a, b = matrices(illum)
    return b @ (a @ (film[:, :3] / film[:, 3:4]).mean(axis=0))


def config(n, illum):
    """A Config whose film has n pixels (n x 1) and the XYZ sensor under `illum`; the scene is K2's."""
    cfg = ref.k2_distant()[0]
    res = (n, 1)
    cam = ref._down_camera(res)
    film = scene.Film(res=res, sensor=capi.RT_SENSOR_XYZ, sensor_illum=illum)
    return scene.Config(f"resolve_{n}", cfg.model, cam, cfg.sampler, film, cfg.integrator, 0, 1)
