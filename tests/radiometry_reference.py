"""Closed-form radiometry in numpy float64: the third leg of the path integrator's checks.

The GPU kernels are compared bit for bit with oracle/rtcore.hpp, which was written by the same hand.  This module
states, independently of both, what the film of a few scenes must converge to: point, distant, quad and disk lights
over a Lambert plane, a point light in an integrating sphere, and mirror / glass spheres in a furnace.  Every
emitter is k * D65.  In the grey cases every albedo is a wavelength-constant sigmoid, so the expected sensor RGB of a
pixel is a geometric scalar times the sensor white W.  The colour cases ("spectral part" below) put a sigmoid that
varies with the wavelength on the floor, the sphere or the mirror and change the film's sensor, so that W becomes
`response(bars, imaging_ratio, f)`: the tables are read at the rounded wavelength, the sigmoid is evaluated at the
continuous one, and throughput is a power of the sigmoid per wavelength.

Nothing here calls the oracle or the product library; `capi` and `scene` are used only to build the descriptors the
renderers are given; the camera rays come from tests/camera_reference.py, the closed-form float64 camera built from
the camera's parameters (not from a descriptor's matrices).

A case is a function returning (scene.Config, mu, vmax, include):
  mu[p, c]    expected film.rgb / film.w of pixel id p (the closed form averaged over an S x S sub-pixel grid),
  vmax[c]     an upper bound on a single sample's value (samples are clamped to [0, 1] before they are added, so the
              closed form only holds while nothing clamps: every case asserts vmax < 1),
  include[p]  False where the sub-samples of a pixel disagree on what they see (surface, lit / shadowed) or where a
              known truncation bias is not negligible; every case asserts that at most 10 % are excluded.
`compare` applies the derived tolerance (a sample lies in [0, vmax] with mean mu, so its variance is at most
mu (vmax - mu), Bhatia-Davis) to the whole frame and to its four quadrants.
"""
import math
from pathlib import Path

import numpy as np

import camera_reference
from computational_ray_tracer_amd import capi, scene

GOLDEN = Path(__file__).resolve().parent / "golden"
CIE_Y_INTEGRAL = 106.856895
RES = (64, 64)
S = 4                      # sub-pixel grid of the footprint average
RHO = 0.5                  # grey albedo: sigmoid c2 = 0, s(0) = 0.5 exactly
FLOAT_ALLOWANCE = 1e-3     # fixed share of mean(mu): float32 accumulation + footprint quadrature
EXCLUDED_MAX = 0.10
POWER_MAX = 0.02           # whole-frame tolerance / mean(mu) that every case must reach
BOUND_SLACK = 1.001        # on vmax: float32 rounding of the estimator, the 1e-4 (1 + max|p|) ray offsets

# ------------------------------------------------------------------------------------------- spectra


TABLES = dict(np.load(GOLDEN / "spectra_tables.npz"))
LAMBDA = np.arange(360, 831, dtype=np.float64)


def _tables():
    z = TABLES
    lam = LAMBDA
    assert np.array_equal(z["CIE_lambda"].astype(np.float64), lam)
    bars = np.stack([z["CIE_X"], z["CIE_Y"], z["CIE_Z"]]).astype(np.float64)
    d = z["CIE_Illum_D6500"].astype(np.float64)
    d65 = np.interp(lam, d[0::2], d[1::2])
    d65 *= CIE_Y_INTEGRAL / np.sum(bars[1] * d65)          # the convention of test_spectra_init_normalisation
    bk = z["GlassBK7_eta"].astype(np.float64)
    bk7 = np.interp(lam, bk[0::2], bk[1::2])
    return bars, d65, bk7


BARS, D65, BK7_ETA = _tables()


def visible_pdf(lam):
    """The documented wavelength pdf 0.0039398042 / cosh^2(0.0072 (lambda - 538)) on [360, 830]."""
    lam = np.asarray(lam, np.float64)
    p = 0.0039398042 / np.cosh(0.0072 * (lam - 538.0)) ** 2
    return np.where((lam >= 360) & (lam <= 830), p, 0.0)


def sample_visible(u):
    """Its inverse CDF (Sampling.h:69-71)."""
    return 538.0 - 138.888889 * np.arctanh(0.85691062 - 1.82750197 * np.asarray(u, np.float64))


def sensor_white(imaging_ratio):
    """W_c = imaging_ratio * sum over the integer nanometres of bar_c * D65: the sensor RGB of radiance 1 * D65 (the
    dense tables are looked up at the rounded wavelength, so the estimator's expectation is this sum)."""
    w = float(imaging_ratio) * (BARS @ D65)
    assert np.allclose(w, (0.95047, 1.0, 1.08883), atol=1e-4), w
    return w


def sample_maxima(imaging_ratio, n=65536, bars=None, envelope=None):
    """(M8, M1): per channel, the largest sensor value one sample of radiance 1 * D65 can take with all eight hero
    wavelengths (u + i/8) alive, and with the first alone after TerminateSecondary (pdf[0] / 8, the others 0).
    `bars`: the sensor's curves (default: the CIE bars).  `envelope`: an upper envelope, a function of the
    continuous wavelength, of the factor f in the radiance D65(round lambda) * f(lambda) (default: 1)."""
    bars = BARS if bars is None else bars
    u = (np.arange(n) + 0.5) / n
    ui = (u[None, :] + np.arange(8)[:, None] / 8.0) % 1.0
    lam = np.clip(sample_visible(ui), 360.0, 830.0)
    k = np.clip(np.rint(lam).astype(int) - 360, 0, 470)
    f = bars[:, k] * D65[k] / visible_pdf(lam) * float(imaging_ratio)      # (3, 8, n)
    if envelope is not None:
        e = np.broadcast_to(envelope(lam), lam.shape)
        assert np.all(e >= 0)
        f = f * e[None]
    m8 = f.mean(axis=1).max(axis=1)
    m1 = f[:, 0, :].max(axis=1)
    assert np.all(np.isfinite(m8)) and np.all(np.isfinite(m1)) and np.all(m1 >= m8)
    return m8 * BOUND_SLACK, m1 * BOUND_SLACK


# ------------------------------------------------------------------------------------------- spectral part

S_RED = (0.0, 0.02, -0.02 * 580)                    # a red edge at 580 nm, about 100 nm wide
S_GREEN = (-4e-4, 0.432, -4e-4 * 540 ** 2 + 2)      # a band around 540 nm: x = 2 - 4e-4 (lambda - 540)^2
SUB = 1024                 # midpoint sub-grid per 1 nm bin (even: a table's knots at integer nm fall on its edges)
ILLUMINANTS = {capi.RT_ILLUM_D65: "CIE_Illum_D6500", capi.RT_ILLUM_A: "CIE_Illum_A",
               capi.RT_ILLUM_D50: "CIE_Illum_D5000", capi.RT_ILLUM_F1: "CIE_Illum_F1",
               capi.RT_ILLUM_F1 + 10: "CIE_Illum_F11"}


def sigmoid(c, lam):
    """The albedo 0.5 + x / (2 sqrt(1 + x^2)), x = (c0 lambda + c1) lambda + c2, in float64 at the continuous
    wavelength, of coefficients rounded to float32 first (what the material descriptor carries)."""
    c0, c1, c2 = (float(np.float32(v)) for v in c)
    lam = np.asarray(lam, np.float64)
    x = (c0 * lam + c1) * lam + c2
    return 0.5 + x / (2.0 * np.sqrt(1.0 + x * x))


def sigmoid_power_sum(c, powers):
    """f(lambda) = sum over `powers` of sigmoid(c, lambda)^p: what a path of several bounces multiplies up."""
    powers = list(powers)
    return lambda lam: sum(sigmoid(c, lam) ** p for p in powers)


def illuminant(which):
    """A named illuminant (RT_ILLUM_*) as a function of the continuous wavelength, built as D65 is in `_tables`:
    linear interpolation of the table, constant beyond its ends, scaled so that sum over the integer nanometres of
    Y * illuminant = CIE_Y_integral."""
    a = TABLES[ILLUMINANTS[which]].astype(np.float64)
    scale = CIE_Y_INTEGRAL / np.sum(BARS[1] * np.interp(LAMBDA, a[0::2], a[1::2]))
    return lambda lam: scale * np.interp(np.asarray(lam, np.float64), a[0::2], a[1::2])


def sensor_bars(sensor, zero_outside=False):
    """The three response curves of a sensor (an index into, or a name of, scene.SENSORS) as a (3, 471) float64
    array on the integer nanometres 360 .. 830.  "xyz" is the CIE bars.  A camera's curves are tabulated on
    380 .. 720 nm; they are interpolated linearly and, not normalised, EXTENDED AS CONSTANTS beyond both ends of the
    table (the reference's FromInterleaved adds the points (359, first) and (831, last)).  That extension is the
    behaviour under test: `zero_outside` builds the other reading, 0 outside the table, which the power tests
    require to fail."""
    name = sensor if isinstance(sensor, str) else scene.SENSORS[sensor]
    assert name in scene.SENSORS
    if name == "xyz":
        return BARS.copy()
    out = []
    for ch in "rgb":
        a = TABLES[f"{name}_{ch}"].astype(np.float64)
        lo, hi = (0.0, 0.0) if zero_outside else (None, None)
        out.append(np.interp(LAMBDA, a[0::2], a[1::2], left=lo, right=hi))
    return np.stack(out)


def bin_integrals(f, sub=SUB):
    """Integral of f over [k - 0.5, k + 0.5] intersected with [360, 830] for the 471 integer nanometres k: the set
    of wavelengths whose table lookups round to k.  Midpoint rule on `sub` points per bin (the end bins have half
    the width)."""
    lo = np.maximum(LAMBDA - 0.5, 360.0)
    hi = np.minimum(LAMBDA + 0.5, 830.0)
    t = (np.arange(sub) + 0.5) / sub
    pts = lo[:, None] + (hi - lo)[:, None] * t[None, :]
    return np.mean(np.broadcast_to(f(pts), pts.shape), axis=1) * (hi - lo)


def response(bars, imaging_ratio, f, table=None, sub=SUB):
    """Expectation of one sample's sensor RGB for the spectral radiance table(round lambda) * f(lambda), `table`
    D65 by default: the wavelength pdf cancels, each of the eight hero wavelengths is distributed with that pdf, so
    E = imaging_ratio * sum_k bars[:, k] table[k] * integral of f over the wavelengths that round to k."""
    table = D65 if table is None else table
    r = float(imaging_ratio) * (bars * table) @ bin_integrals(f, sub)
    fine = float(imaging_ratio) * (bars * table) @ bin_integrals(f, 2 * sub)
    assert np.all(np.abs(fine - r) <= 1e-9 * np.abs(fine)), (r, fine)
    return r


def bin_envelope(f, half=0.5, m=17):
    """An upper envelope of f for `sample_maxima`: at lambda, the largest f on a grid over lambda +- half nm, which
    covers the gaps of the scan over u (they are below 0.1 nm wherever a bar is not negligible)."""
    d = np.linspace(-half, half, m)
    return lambda lam: np.max(np.stack([f(np.clip(np.asarray(lam, np.float64) + x, 360.0, 830.0)) for x in d]), axis=0)


def sigmoid_power_sum_envelope(c, powers):
    """The same sum over the envelope of the sigmoid: an upper envelope of the sum, which grows with the sigmoid."""
    powers = list(powers)
    env = bin_envelope(lambda lam: sigmoid(c, lam))
    return lambda lam: sum(env(lam) ** p for p in powers)


# ------------------------------------------------------------------------------------------- camera


def camera_rays(cfg, offsets):
    """World-space float64 rays of every pixel id at the sub-pixel `offsets` (k, 2) in [0, 1]^2: (origin (3,),
    directions (n_pixels, k, 3)).  Raster x = id % resX, y = resY - floor(id / resX) (DESIGN §5 "Pixel y"); the box
    filter of radius 0.5 spreads a pixel's samples over [x, x + 1] x [y, y + 1]."""
    d = cfg.camera.desc()
    assert d.type == capi.RT_CAMERA_PERSPECTIVE and d.lens_radius == 0
    assert cfg.film.filter == capi.RT_FILTER_BOX and tuple(cfg.film.filter_radius) == (0.5, 0.5)
    assert tuple(cfg.camera.res) == tuple(cfg.film.res)
    px, py = camera_reference.pixel_xy(np.arange(cfg.film.res[0] * cfg.film.res[1]), cfg.film.res)
    offsets = np.asarray(offsets, np.float64)
    o, w = camera_reference.world_ray(cfg.camera, px[:, None] + offsets[None, :, 0], py[:, None] + offsets[None, :, 1])
    return o[0, 0].copy(), w


def _midpoints(s=S):
    g = (np.arange(s) + 0.5) / s
    return np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(-1, 2)


def _lattice(s=S):
    """The footprint's (s + 1)^2 lattice, corners and edges included: what a pixel sees is classified on it, so a
    pixel whose lattice points all lie inside (or all outside) a convex outline lies inside (outside) it entirely."""
    g = np.arange(s + 1) / s
    return np.stack(np.meshgrid(g, g, indexing="xy"), -1).reshape(-1, 2)


# ------------------------------------------------------------------------------------------- comparison


def quadrants(res):
    """Boolean masks over pixel ids: the whole frame and its four quadrants (rows = id // resX)."""
    rx, ry = res
    ids = np.arange(rx * ry)
    col, row = ids % rx, ids // rx
    out = {"frame": np.ones(rx * ry, bool)}
    for name, m in (("q00", (col < rx // 2) & (row < ry // 2)), ("q10", (col >= rx // 2) & (row < ry // 2)),
                    ("q01", (col < rx // 2) & (row >= ry // 2)), ("q11", (col >= rx // 2) & (row >= ry // 2))):
        out[name] = m
    return out


def tolerance(mu, vmax, spp):
    """5 standard errors of the region's mean at the Bhatia-Davis variance bound, plus the fixed float allowance."""
    n = len(mu)
    var = np.sum(mu * (vmax[None, :] - mu), axis=0) / spp
    return 5.0 * np.sqrt(np.maximum(var, 0.0)) / n + FLOAT_ALLOWANCE * mu.mean(axis=0)


def compare(film, mu, vmax, include, spp, res=RES):
    """Rows (region, got[3], want[3], tol[3], ok) of the closed-form comparison of a film [n, 4]; pixels expected to
    be exactly zero are compared with == (row "zero")."""
    film = np.asarray(film, np.float64)
    assert film.shape == (res[0] * res[1], 4) and np.all(film[:, 3] == spp), "every pixel holds spp samples"
    img = film[:, :3] / film[:, 3:4]
    rows = []
    zero = include & np.all(mu == 0.0, axis=1)
    if zero.any():
        worst = img[zero].max(axis=0)
        rows.append(("zero", worst, np.zeros(3), np.zeros(3), bool(np.all(img[zero] == 0.0))))
    for name, m in quadrants(res).items():
        r = m & include
        if not r.any():
            continue
        got, want = img[r].mean(axis=0), mu[r].mean(axis=0)
        tol = tolerance(mu[r], vmax, spp)
        rows.append((name, got, want, tol, bool(np.all(np.abs(got - want) <= tol))))
    return rows


def passes(rows):
    return all(r[4] for r in rows)


def deviation(rows):
    """max |got - mu| / tol over the regions and channels with a tolerance: a recorded figure, not a threshold."""
    return max(float(np.max(np.abs(g - w) / t)) for _, g, w, t, _ in rows if np.all(t > 0))


def report(rows):
    return "\n".join(f"{n:6s} got {np.array2string(g, precision=6)} want {np.array2string(w, precision=6)} "
                     f"tol {np.array2string(t, precision=6)} {'ok' if ok else 'FAIL'}" for n, g, w, t, ok in rows)


def _finish(name, cfg, mu, vmax, include, spp):
    """The preconditions every case asserts on its own inputs."""
    vmax = np.asarray(vmax, np.float64)
    assert mu.shape == (cfg.film.res[0] * cfg.film.res[1], 3) and np.all(np.isfinite(mu)) and np.all(mu >= 0)
    assert np.all(vmax < 1.0), f"{name}: a sample can clamp, vmax {vmax}"
    assert np.all(mu[include] <= vmax[None, :]), f"{name}: vmax is no bound of mu"
    excluded = 1.0 - include.mean()
    assert excluded <= EXCLUDED_MAX, f"{name}: {excluded:.3f} of the pixels excluded"
    power = tolerance(mu[include], vmax, spp) / mu[include].mean(axis=0)
    assert np.all(power <= POWER_MAX), f"{name}: whole-frame tolerance {power} of the mean"
    assert cfg.index_end - cfg.index_begin == spp == cfg.sampler.spp()
    return cfg, mu, vmax, include


# ------------------------------------------------------------------------------------------- scenes

FAR_TRIANGLE = np.array([[1e4, 1e4, 1e4], [1e4 + 1, 1e4, 1e4], [1e4, 1e4 + 1, 1e4]], np.float64)
FLOOR_HALF = 4000.0
EYE_HEIGHT = 1000.0
VIEW_HALF = 200.0              # the floor square the camera sees, about


def _model(tris, tri_material, materials, lights=(), shapes=()):
    """World-space triangles (nt, 3, 3), object space = world with y and z swapped."""
    tris = np.asarray(tris, np.float64)
    pos, nrm, idx = scene._flat_mesh(tris[:, :, [0, 2, 1]])
    m = scene.TriModel(pos, nrm, idx, rigid=np.eye(4), tri_material=np.asarray(tri_material, np.int32))
    m.materials = list(materials)
    m.lights = list(lights)
    m.shapes = list(shapes)
    return m


def _floor_tris(n, x_lines=()):
    """The floor y = 0, |x|, |z| <= FLOOR_HALF, as n x n x 2 triangles.  `x_lines`: further grid lines x = const that
    are no line of the n x n grid (a seam between two materials that a coarse grid would not hold); each adds a column."""
    g = np.linspace(-FLOOR_HALF, FLOOR_HALF, n + 1)
    gx = g
    for x in x_lines:
        if not np.any(np.abs(gx - x) <= 1e-9 * FLOOR_HALF):
            assert -FLOOR_HALF < x < FLOOR_HALF
            gx = np.sort(np.append(gx, x))
    t = []
    for i in range(len(gx) - 1):
        for j in range(n):
            a, b = (gx[i], 0.0, g[j]), (gx[i + 1], 0.0, g[j])
            c, d = (gx[i + 1], 0.0, g[j + 1]), (gx[i], 0.0, g[j + 1])
            t += [(a, c, b), (a, d, c)]
    return np.array(t)


def _config(name, model, camera, spp, kind, max_depth, res=RES, film=None, albedo_rgb=None):
    side = int(round(math.sqrt(spp)))
    assert side * side == spp
    film = scene.Film(res=res) if film is None else film
    integ = scene.Integrator(kind, max_depth=max_depth)
    if albedo_rgb is not None:
        integ.albedo_rgb = tuple(albedo_rgb)
    return scene.Config(name, model, camera, scene.StratifiedSampler(side, side, True, 0), film, integ, 0, spp)


def _film(sensor="xyz", illum=capi.RT_ILLUM_D65, exposure=1.0):
    """The film of a case: the sensor by name.  The sensor illuminant only enters the resolve matrices, never the
    accumulated sensor RGB; the colour cases set it as a user of that sensor would.  `exposure` (a power of two)
    scales the imaging ratio."""
    film = scene.Film(res=RES, sensor=scene.SENSORS.index(sensor), sensor_illum=illum)
    film.imaging_ratio = float(np.float32(film.imaging_ratio) * np.float32(exposure))
    return film


def _per_rho(film, albedo):
    """(w, m8): expected and largest sensor RGB of the radiance D65 * rho(lambda), both divided by RHO, so that the
    grey formulas `RHO * ... * w` hold for a coloured albedo as they stand.  Grey on the XYZ sensor: the sensor white
    and `sample_maxima`, as before."""
    if albedo is None and film.sensor == capi.RT_SENSOR_XYZ:
        return sensor_white(film.imaging_ratio), sample_maxima(film.imaging_ratio)[0]
    bars = sensor_bars(film.sensor)
    c = scene.grey_sigmoid(RHO) if albedo is None else albedo
    f = lambda lam: sigmoid(c, lam)
    return (response(bars, film.imaging_ratio, f) / RHO,
            sample_maxima(film.imaging_ratio, bars=bars, envelope=bin_envelope(f))[0] / RHO)


def _fov(slope):
    """PerspectiveCamera(near = 1) applies tan(fov / 2) twice (Cameras.h:255 and :305-307): the frame's half-width
    at distance 1 is tan^2(fov / 2).  The reference rays come from the descriptor's matrices either way."""
    return 2.0 * math.degrees(math.atan(math.sqrt(slope)))


def _down_camera(res=RES):
    fov = _fov(VIEW_HALF / EYE_HEIGHT)
    return scene.PerspectiveCamera(near=1.0, far=5000.0, fov=fov, position=(0.0, EYE_HEIGHT, 0.0), look=(0, -1, 0),
                                   worldup=(0, 0, 1), res=res, aspect_fix=True)


def _floor_points(cfg, offsets):
    """Where the camera rays meet y = 0: (n_pixels, k, 3)."""
    o, w = camera_rays(cfg, offsets)
    assert np.all(w[..., 1] < 0)
    t = -o[1] / w[..., 1]
    x = o[None, None, :] + t[..., None] * w
    assert np.all(np.abs(x[..., [0, 2]]) < FLOOR_HALF)
    return x


def _view_box(cfg):
    """Bounding rectangle (xmin, xmax, zmin, zmax) of every footprint on the floor."""
    x = _floor_points(cfg, _lattice())
    box = x[..., 0].min(), x[..., 0].max(), x[..., 2].min(), x[..., 2].max()
    assert np.allclose(box, (-VIEW_HALF, VIEW_HALF, -VIEW_HALF, VIEW_HALF), atol=2 * VIEW_HALF / cfg.film.res[1] + 1e-3)
    return box


def _outside_frustum(cfg, pts):
    """True when no world point of `pts` (n, 3) below the eye projects into the raster (the camera cannot see it)."""
    cam = cfg.camera
    R = camera_reference.frame(cam.look, cam.worldup)
    pc = (np.asarray(pts, np.float64) - np.asarray(cam.position, np.float64)) @ R.T          # camera space
    assert np.all(pc[:, 2] > 0)
    rx, ry = cfg.film.res
    corners = camera_reference.camera_ray(cam, np.array([0.0, rx]), np.array([1.0, ry + 1.0]))[1]
    lo = np.minimum(corners[0, :2] / corners[0, 2], corners[1, :2] / corners[1, 2])
    hi = np.maximum(corners[0, :2] / corners[0, 2], corners[1, :2] / corners[1, 2])
    s = pc[:, :2] / pc[:, 2:3]
    return bool(np.all(s[:, 0] < lo[0]) or np.all(s[:, 0] > hi[0]) or
                np.all(s[:, 1] < lo[1]) or np.all(s[:, 1] > hi[1]))


TESSELLATED_N = 48         # the floor of the "tessellated" cases: a BFS queue bound above 16, the LDS + HBM FIFO (QCAP 0)


def floor_cells(tessellated):
    """The floor's cells per side: False -> 1 (a single leaf), True -> TESSELLATED_N, an int -> itself (a coarser
    tessellation keeps every closed form, which is of the plane, and selects another traversal instantiation)."""
    if isinstance(tessellated, (bool, np.bool_)):
        return TESSELLATED_N if tessellated else 1
    n = int(tessellated)
    assert n == tessellated and n >= 1, tessellated
    return n


def _floor_model(tessellated, extra_tris=(), extra_mats=(), materials=(), lights=(), shapes=(), albedo=None, x_lines=()):
    tris = _floor_tris(floor_cells(tessellated), x_lines)
    mats = [0] * len(tris)
    if len(extra_tris):
        tris = np.concatenate([tris, np.asarray(extra_tris, np.float64)])
        mats += list(extra_mats)
    floor = scene.grey_sigmoid(RHO) if albedo is None else albedo
    return _model(tris, mats, [(floor, 0.0)] + list(materials), lights, shapes)


# ------------------------------------------------------------------------------------------- K1, K1s, K2

POINT_P = np.array([600.0, 400.0, -300.0])


def _point_irradiance(x, p, n):
    """cos(theta) / d^2 at surface points x (..., 3) with normals n (..., 3) for a point light at p."""
    v = p - x
    d2 = np.sum(v * v, axis=-1)
    return np.maximum(np.sum(v * n, axis=-1), 0.0) / (d2 * np.sqrt(d2))


def _point_bound(cfg, p):
    """max of cos / d^2 = h / d^3 over the seen floor rectangle: d >= its distance from the light."""
    x0, x1, z0, z1 = _view_box(cfg)
    gap = np.hypot(max(p[0] - x1, x0 - p[0], 0.0), max(p[2] - z1, z0 - p[2], 0.0))
    return p[1] / (p[1] ** 2 + gap ** 2) ** 1.5


def k1_point(tessellated=False, spp=256, albedo=None, sensor="xyz", illum=capi.RT_ILLUM_D65):
    """K1: a point light of intensity I * D65 over the Lambert floor, L = rho / pi * I cos(theta) / d^2."""
    inten = 2.0e6
    lights = [dict(type=capi.RT_LIGHT_POINT, p=tuple(POINT_P), scale=inten)]
    cfg = _config("k1_point", _floor_model(tessellated, lights=lights, albedo=albedo), _down_camera(), spp,
                  capi.RT_INTEGRATOR_PATH, 1, film=_film(sensor, illum))
    w, m8 = _per_rho(cfg.film, albedo)
    x = _floor_points(cfg, _midpoints())
    k = RHO / math.pi * inten * _point_irradiance(x, POINT_P, np.array([0.0, 1.0, 0.0])).mean(axis=1)
    mu = k[:, None] * w[None, :]
    vmax = RHO / math.pi * inten * _point_bound(cfg, POINT_P) * m8
    return _finish("k1_point", cfg, mu, vmax, np.ones(len(mu), bool), spp)


SHADOW_DISK_C = np.array([320.0, 200.0, -160.0])   # halfway from the light to the floor point (40, 0, -20)
SHADOW_DISK_R = 60.0


def k1s_point_shadow(spp=256):
    """K1s: K1 plus a horizontal diffuse Disk between the light and the floor, outside the camera's view.  At
    max_depth 1 a pixel wholly in the umbra is exactly 0; lit pixels are K1's."""
    inten = 2.0e6
    lights = [dict(type=capi.RT_LIGHT_POINT, p=tuple(POINT_P), scale=inten)]
    disk = scene.Disk(scene.translate(tuple(SHADOW_DISK_C)), 0, height=0.0, inner_radius=0.0,
                      outer_radius=SHADOW_DISK_R)                  # object +z -> world +y: horizontal
    cfg = _config("k1s_point_shadow", _floor_model(False, lights=lights, shapes=[disk]), _down_camera(), spp,
                  capi.RT_INTEGRATOR_PATH, 1)
    ang = np.linspace(0, 2 * math.pi, 64, endpoint=False)
    rim = SHADOW_DISK_C + SHADOW_DISK_R * np.stack([np.cos(ang), 0 * ang, np.sin(ang)], -1)
    assert _outside_frustum(cfg, rim), "the camera sees the occluder"
    w = sensor_white(cfg.film.imaging_ratio)
    m8, _ = sample_maxima(cfg.film.imaging_ratio)

    def disk_radius(x):          # where the segment x -> light crosses the disk's plane, distance from its centre
        t = (SHADOW_DISK_C[1] - x[..., 1]) / (POINT_P[1] - x[..., 1])
        q = x + t[..., None] * (POINT_P - x)
        return np.linalg.norm(q - SHADOW_DISK_C, axis=-1)
    rl = disk_radius(_floor_points(cfg, _lattice()))
    eps = 1e-3                   # the shadow ray starts 1e-4 (1 + max|p|) above the floor: the outline moves by < 0.1
    umbra = np.all(rl < SHADOW_DISK_R * (1 - eps), axis=1)
    lit = np.all(rl > SHADOW_DISK_R * (1 + eps), axis=1)
    assert umbra.mean() > 0.1 and lit.mean() > 0.5
    x = _floor_points(cfg, _midpoints())
    k = RHO / math.pi * inten * _point_irradiance(x, POINT_P, np.array([0.0, 1.0, 0.0])).mean(axis=1)
    mu = np.where(umbra[:, None], 0.0, k[:, None] * w[None, :])
    vmax = RHO / math.pi * inten * _point_bound(cfg, POINT_P) * m8
    return _finish("k1s_point_shadow", cfg, mu, vmax, umbra | lit, spp)


K2_E = 2.5
K2_DIR = np.array([0.3, 0.8, 0.2])
K2_GEOMETRY = K2_E * K2_DIR[1] / np.linalg.norm(K2_DIR) / math.pi          # E cos(theta) / pi


def k2_distant(tessellated=False, spp=256, albedo=None, sensor="xyz", illum=capi.RT_ILLUM_D65):
    """K2: a distant light of irradiance E * D65 from an oblique direction, L = rho / pi * E cos(theta), uniform.
    With a coloured floor: E cos(theta) / pi * response(bars, imaging_ratio, rho)."""
    e = K2_E
    d = K2_DIR
    lights = [dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(d), scale=e)]
    cfg = _config("k2_distant", _floor_model(tessellated, lights=lights, albedo=albedo), _down_camera(), spp,
                  capi.RT_INTEGRATOR_PATH, 1, film=_film(sensor, illum))
    w, m8 = _per_rho(cfg.film, albedo)
    k = RHO / math.pi * e * d[1] / np.linalg.norm(d)
    n = cfg.film.res[0] * cfg.film.res[1]
    mu = np.tile(k * w, (n, 1))
    return _finish("k2_distant", cfg, mu, k * m8, np.ones(n, bool), spp)


# ------------------------------------------------------------------------------------------- K3 quad light

QUAD_H = 450.0
QUAD_X = (140.0, 380.0)
QUAD_Z = (0.0, 240.0)


def polygon_irradiance(x, verts, n):
    """Lambert's formula: the irradiance at x (..., 3), normal n, of a unit-radiance polygon `verts` (m, 3) wholly
    above the horizon: E = 1/2 |sum over the edges of theta_i (gamma_i . n)|, theta_i the angle the edge subtends,
    gamma_i the unit normal of the plane through x and the edge.  Exact."""
    v = verts[None, :, :] - np.asarray(x, np.float64).reshape(-1, 1, 3)
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    v2 = np.roll(v, -1, axis=1)
    cr = np.cross(v, v2)
    sn = np.linalg.norm(cr, axis=-1)
    theta = np.arctan2(sn, np.sum(v * v2, axis=-1))
    e = 0.5 * np.abs(np.sum(theta * (cr @ n) / sn, axis=1))
    return e.reshape(np.shape(x)[:-1])


def quad_irradiance_bruteforce(x, p, e1, e2, nl, n, m=1024):
    """Midpoint quadrature of cos cos / d^2 over the parallelogram p + u e1 + v e2 (normal nl)."""
    g = (np.arange(m) + 0.5) / m
    y = p + g[:, None, None] * e1 + g[None, :, None] * e2
    v = y - x
    d2 = np.sum(v * v, -1)
    f = np.maximum(v @ n, 0) * np.maximum(-(v @ nl), 0) / (d2 * d2)
    return f.mean() * np.linalg.norm(np.cross(e1, e2))


QUAD_SEEN_SHIFT = -120.0       # along x: moves a corner of the light into the camera's view


def k3_quad(mis=False, max_depth=1, tessellated=False, seen=False, spp=256, albedo=None, sensor="xyz",
            illum=capi.RT_ILLUM_D65):
    """K3: a quad light Le * D65 above the floor and parallel to it, as two emissive triangles and an RT_LIGHT_QUAD.
    The plane is open: a bounce never returns to it, so every depth has the depth-1 expectation rho * F(x) * Le with
    pi F = Lambert's polygon formula.  One NEE sample is rho / pi Le G A (times w_l <= 1 with MIS); with MIS a bounce
    that hits the light adds rho Le w_b, w_b = 1 / (1 + (p_l / p_b)^2) and p_l / p_b = pi / (G A).
    `seen`: the light is moved under the camera, which then looks at its back: emitters are one-sided, so a pixel
    wholly on the light is exactly 0, and the floor pixels keep their closed form (nothing hides the light's front
    from the floor).  A coloured floor changes only the colour factor: no light reaches the floor twice, so the
    albedo enters to the first power at every depth."""
    le = 16.0 if albedo is None else 10.0        # rho peaks near 0.95, not 0.5: a dimmer light keeps vmax below 1
    qx = (QUAD_X[0] + QUAD_SEEN_SHIFT, QUAD_X[1] + QUAD_SEEN_SHIFT) if seen else QUAD_X
    p = np.array([qx[1], QUAD_H, QUAD_Z[0]])
    e1, e2 = np.array([0.0, 0.0, QUAD_Z[1] - QUAD_Z[0]]), np.array([qx[0] - qx[1], 0.0, 0.0])
    nl = np.array([0.0, -1.0, 0.0])
    assert np.allclose(np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2)), nl)
    a, b, c, d = p, p + e1, p + e1 + e2, p + e2
    ltris = np.array([(a, b, c), (a, c, d)])                      # wound so that the geometric normal is nl
    assert np.allclose(np.cross(b - a, c - a) / np.linalg.norm(np.cross(b - a, c - a)), nl)
    lights = [dict(type=capi.RT_LIGHT_QUAD, p=tuple(p), e1=tuple(e1), e2=tuple(e2), n=tuple(nl), material=1)]
    model = _floor_model(tessellated, ltris, [1, 1], [((0.0, 0.0, 0.0), le)], lights, albedo=albedo)
    kind = capi.RT_INTEGRATOR_PATH_MIS if mis else capi.RT_INTEGRATOR_PATH
    cfg = _config("k3_quad", model, _down_camera(), spp, kind, max_depth, film=_film(sensor, illum))
    verts = np.array([a, b, c, d])
    assert seen or _outside_frustum(cfg, verts), "the camera sees the light"
    w, m8 = _per_rho(cfg.film, albedo)
    x = _floor_points(cfg, _midpoints())
    up = np.array([0.0, 1.0, 0.0])
    form = polygon_irradiance(x, verts, up).mean(axis=1) / math.pi
    mu = (RHO * le * form)[:, None] * w[None, :]
    include = np.ones(len(mu), bool)
    if seen:     # where the camera rays cross the light's plane: inside its rectangle they end on its back
        o, d = camera_rays(cfg, _lattice())
        y = o + ((QUAD_H - o[1]) / d[..., 1])[..., None] * d
        eps = 1e-3

        def inside(margin):
            return ((y[..., 0] > qx[0] - margin) & (y[..., 0] < qx[1] + margin) &
                    (y[..., 2] > QUAD_Z[0] - margin) & (y[..., 2] < QUAD_Z[1] + margin))
        back, floor = np.all(inside(-eps), axis=1), ~np.any(inside(eps), axis=1)
        assert back.mean() > 0.1 and floor.mean() > 0.5
        mu = np.where(back[:, None], 0.0, mu)
        include = back | floor
    # G = h^2 / d^4 between parallel planes, d >= the distance of the seen floor rectangle from the light's
    x0, x1, z0, z1 = _view_box(cfg)
    gap = np.hypot(max(qx[0] - x1, x0 - qx[1], 0.0), max(QUAD_Z[0] - z1, z0 - QUAD_Z[1], 0.0))
    g = QUAD_H ** 2 / (QUAD_H ** 2 + gap ** 2) ** 2 * np.linalg.norm(np.cross(e1, e2)) / math.pi
    bound = RHO * le * (g + (g * g / (1 + g * g) if mis else 0.0))
    return _finish("k3_quad", cfg, mu, bound * m8, include, spp)


# ------------------------------------------------------------------------------------------- K4 disk light

DISK_C = np.array([330.0, 420.0, 110.0])
DISK_R = 110.0
DISK_TILT = -30.0          # about z, after the half turn about x that points the disk down: its normal leans to -x


def _disk_frame(tilt=DISK_TILT, centre=DISK_C):
    """Rigid transform of the emissive Disk (emits along object +z) and, from it, centre, unit normal and two unit
    in-plane axes in world space: a half turn about x points the disk down, then the tilt about z."""
    rigid = scene.translate(tuple(centre)) @ scene.rotate(tilt, (0, 0, 1)) @ scene.rotate(180.0, (1, 0, 0))
    o2r = rigid @ scene.PERM_YZ
    return rigid, o2r[:3, 3], o2r[:3, 2], o2r[:3, 0], o2r[:3, 1]


def disk_irradiance_quadrature(x, c, nl, ax, ay, radius, n, m=512):
    """Polar midpoint quadrature (m radii x m angles) of cos cos / d^2 over the disk, unit radiance, at one point x."""
    r = (np.arange(m) + 0.5) / m * radius
    ph = (np.arange(m) + 0.5) / m * 2 * math.pi
    y = c + r[:, None, None] * (np.cos(ph)[None, :, None] * ax + np.sin(ph)[None, :, None] * ay)
    v = y - x
    d2 = np.sum(v * v, -1)
    f = np.maximum(v @ n, 0) * np.maximum(-(v @ nl), 0) / (d2 * d2)
    return float(np.sum(f * r[:, None]) * (radius / m) * (2 * math.pi / m))


def disk_irradiance_contour(x, c, nl, ax, ay, radius, n, m=128):
    """The same irradiance as a contour integral (Stokes; Lambert's formula in the limit of many edges):
    E = 1/2 |n . closed integral of (r x dr) / |r|^2|, r from x to the rim, by the periodic midpoint rule, which
    converges geometrically.  The disk must be wholly above x's horizon and face x.  One float per point of x, so
    a whole film is cheap; `disk_irradiance_quadrature` is the definition it is checked against."""
    ph = (np.arange(m) + 0.5) / m * 2 * math.pi
    rim = c + radius * (np.cos(ph)[:, None] * ax + np.sin(ph)[:, None] * ay)
    drim = radius * (-np.sin(ph)[:, None] * ax + np.cos(ph)[:, None] * ay) * (2 * math.pi / m)
    xs = np.asarray(x, np.float64).reshape(-1, 1, 3)
    r = rim[None] - xs
    assert np.all(r @ n > 0) and np.all(r @ nl < 0)
    integrand = np.cross(r, drim[None]) / np.sum(r * r, -1, keepdims=True)
    return (0.5 * np.abs(integrand.sum(axis=1) @ n)).reshape(np.shape(x)[:-1])


def k4_disk(mis=False, max_depth=1, spp=256):
    """K4: an emissive Disk shape, tilted by 30 degrees and translated (rigid, not scaled), as an RT_LIGHT_DISK."""
    le = 15.0
    rigid, c, nl, ax, ay = _disk_frame()
    assert abs(np.linalg.norm(nl) - 1) < 1e-12 and nl[1] < 0
    disk = scene.Disk(rigid, 1, height=0.0, inner_radius=0.0, outer_radius=DISK_R)
    lights = [dict(type=capi.RT_LIGHT_DISK, shape=0)]
    model = _floor_model(False, materials=[((0.0, 0.0, 0.0), le)], lights=lights, shapes=[disk])
    kind = capi.RT_INTEGRATOR_PATH_MIS if mis else capi.RT_INTEGRATOR_PATH
    cfg = _config("k4_disk", model, _down_camera(), spp, kind, max_depth)
    ang = np.linspace(0, 2 * math.pi, 64, endpoint=False)
    rim = c + DISK_R * (np.cos(ang)[:, None] * ax + np.sin(ang)[:, None] * ay)
    assert _outside_frustum(cfg, rim), "the camera sees the light"
    w = sensor_white(cfg.film.imaging_ratio)
    m8, _ = sample_maxima(cfg.film.imaging_ratio)
    up = np.array([0.0, 1.0, 0.0])
    x = _floor_points(cfg, _midpoints())
    e = disk_irradiance_contour(x, c, nl, ax, ay, DISK_R, up)
    # the definition, at the four corner pixels and the centre one: 512 x 512 polar midpoint quadrature
    rx, ry = cfg.film.res
    for pid in (0, rx - 1, rx * (ry - 1), rx * ry - 1, rx * (ry // 2) + rx // 2):
        q = disk_irradiance_quadrature(x[pid, 0], c, nl, ax, ay, DISK_R, up)
        assert abs(q - e[pid, 0]) <= 1e-6 * q, (pid, q, e[pid, 0])
    mu = (RHO / math.pi * le * e.mean(axis=1))[:, None] * w[None, :]
    # G = cos cos / d^2 <= 1 / d^2, d >= the distance of the seen floor rectangle from the rim's bounding box
    x0, x1, z0, z1 = _view_box(cfg)
    gap = np.hypot(max(rim[:, 0].min() - x1, x0 - rim[:, 0].max(), 0.0),
                   max(rim[:, 2].min() - z1, z0 - rim[:, 2].max(), 0.0))
    g = 1.0 / (rim[:, 1].min() ** 2 + gap ** 2) * (math.pi * DISK_R ** 2) / math.pi
    bound = RHO * le * (g + (g * g / (1 + g * g) if mis else 0.0))
    return _finish("k4_disk", cfg, mu, bound * m8, np.ones(len(mu), bool), spp)


# ------------------------------------------------------------------------------------------- K5 integrating sphere

SPHERE_R = 100.0
SPHERE_LIGHT = np.array([20.0, -15.0, 10.0])
SPHERE_EYE = np.array([0.0, 0.0, -60.0])


K5_COLOUR_INTENSITY = 4.0e3


def k5_direct(cfg):
    """cos / d^2 of the point light at what every pixel sees of the sphere's inside, footprint average."""
    o, d = camera_rays(cfg, _midpoints())
    bq = d @ o
    t = -bq + np.sqrt(bq * bq - (o @ o - SPHERE_R ** 2))           # the far root: the eye is inside
    x = o + t[..., None] * d
    return _point_irradiance(x, SPHERE_LIGHT, -x / SPHERE_R).mean(axis=1)


def k5_sphere(max_depth=1, spp=256, albedo=None):
    """K5: camera and an off-centre point light inside a diffuse Sphere shape of radius r.  The form factor between
    any two elements of a sphere's inside is dA / (4 pi r^2), so every bounce spreads its flux evenly:
    L(x) = rho / pi [I cos / d^2 + I / r^2 sum_{k=1..D-1} rho^k] with NEE at depths 0 .. D - 1 (max_depth = D).
    With a coloured sphere rho is a function of the wavelength and the sum holds per wavelength, so
    mu = I / pi [direct * response(rho) + 1 / r^2 sum_{k=1..D-1} response(rho^(k+1))]: the one closed form here in
    which throughput is a power of the albedo per wavelength, not of a colour."""
    inten = 1.2e4 if albedo is None else K5_COLOUR_INTENSITY
    lights = [dict(type=capi.RT_LIGHT_POINT, p=tuple(SPHERE_LIGHT), scale=inten)]
    model = _model([FAR_TRIANGLE], [0], [(scene.grey_sigmoid(RHO) if albedo is None else albedo, 0.0)], lights,
                   [scene.Sphere(np.eye(4), 0, radius=SPHERE_R)])
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=_fov(0.8), position=tuple(SPHERE_EYE), look=(0, 0, 1),
                                  worldup=(0, 1, 0), res=RES, aspect_fix=True)
    cfg = _config("k5_sphere", model, cam, spp, capi.RT_INTEGRATOR_PATH, max_depth)
    direct = k5_direct(cfg)
    dmin = SPHERE_R - np.linalg.norm(SPHERE_LIGHT)
    if albedo is not None:
        ir = cfg.film.imaging_ratio
        first = response(BARS, ir, sigmoid_power_sum(albedo, [1]))
        later = response(BARS, ir, sigmoid_power_sum(albedo, range(2, max_depth + 1))) if max_depth > 1 else 0.0
        mu = inten / math.pi * (direct[:, None] * first[None, :] + later / SPHERE_R ** 2)
        # each depth's NEE sample is at most rho^(k+1) / pi I / d_min^2 at its wavelength
        m8, _ = sample_maxima(ir, envelope=sigmoid_power_sum_envelope(albedo, range(1, max_depth + 1)))
        return _finish("k5_sphere", cfg, mu, inten / math.pi / dmin ** 2 * m8, np.ones(len(mu), bool), spp)
    w = sensor_white(cfg.film.imaging_ratio)
    m8, _ = sample_maxima(cfg.film.imaging_ratio)
    bounces = sum(RHO ** k for k in range(1, max_depth)) / SPHERE_R ** 2
    mu = (RHO / math.pi * inten * (direct + bounces))[:, None] * w[None, :]
    # each depth's NEE sample is at most rho^(k+1) / pi I / d_min^2, d_min = r - |light|
    bound = inten / math.pi / dmin ** 2 * sum(RHO ** (k + 1) for k in range(max_depth))
    return _finish("k5_sphere", cfg, mu, bound * m8, np.ones(len(mu), bool), spp)


# ------------------------------------------------------------------------------------------- K6 furnace

BOX_HALF = 400.0
FURNACE_R = 100.0
FURNACE_EYE = np.array([0.0, 0.0, -350.0])
FURNACE_DEPTH = 12
LOST_MAX = 1e-4


def fr_dielectric(cos_i, eta):
    """pbrt's unpolarised FrDielectric for a ray arriving from outside (cos_i >= 0, eta > 1), float64."""
    cos_i = np.clip(cos_i, 0.0, 1.0)
    sin2_t = (1 - cos_i * cos_i) / (eta * eta)
    cos_t = np.sqrt(np.maximum(0.0, 1 - sin2_t))
    r_parl = (eta * cos_i - cos_t) / (eta * cos_i + cos_t)
    r_perp = (cos_i - eta * cos_t) / (cos_i + eta * cos_t)
    return (r_parl * r_parl + r_perp * r_perp) / 2


def _box_tris(h):
    c = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64)
    faces = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    t = []
    for a, b, cc, d in faces:
        t += [(c[a], c[b], c[cc]), (c[a], c[cc], c[d])]
    t = np.array(t)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    flip = np.einsum("ij,ij->i", nrm, -t.mean(axis=1)) < 0        # every face looks at the centre
    t[flip] = t[flip][:, [0, 2, 1]]
    return t


def k6_furnace(kind="mirror", spp=256, reflectance=None, sensor="xyz", illum=capi.RT_ILLUM_D65):
    """K6: a closed box of 12 inward-facing triangles emitting L0 * D65, no light records; camera and one Sphere
    inside; PATH, max_depth 12.  A pixel that misses the sphere sees L0 W; the mirror (R = 0.9) 0.9 L0 W; glass
    (constant eta 1.5, or eta 0 = BK7 with TerminateSecondary) L0 W, because the 1 / eta'^2 factors cancel.  A path
    that enters the glass and is reflected inside 11 times is cut off: probability (1 - F) F^11, F the entry
    reflectance, the same at every interface of a sphere; pixels where it can exceed 1e-4 are excluded.
    `reflectance`: a sigmoid R(lambda) on the mirror instead of 0.9; pixels on the sphere then expect
    L0 * response(R), the others L0 * response(1)."""
    assert kind in ("mirror", "glass", "bk7") and (reflectance is None or kind == "mirror")
    film = _film(sensor, illum)
    bars = sensor_bars(film.sensor)
    m8, m1 = sample_maxima(film.imaging_ratio, bars=bars)
    l0 = 0.9 / (m1 if kind == "bk7" else m8).max()
    mats = [((0.0, 0.0, 0.0), l0),
            {"mirror": (scene.grey_sigmoid(0.9) if reflectance is None else reflectance, 0.0, capi.RT_MAT_MIRROR, 0.0),
             "glass": ((0.0, 0.0, 0.0), 0.0, capi.RT_MAT_DIELECTRIC, 1.5),
             "bk7": ((0.0, 0.0, 0.0), 0.0, capi.RT_MAT_DIELECTRIC, 0.0)}[kind]]
    model = _model(_box_tris(BOX_HALF), [0] * 12, mats, (), [scene.Sphere(np.eye(4), 1, radius=FURNACE_R)])
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=_fov(0.42), position=tuple(FURNACE_EYE), look=(0, 0, 1),
                                  worldup=(0, 1, 0), res=RES, aspect_fix=True)
    cfg = _config(f"k6_furnace_{kind}", model, cam, spp, capi.RT_INTEGRATOR_PATH, FURNACE_DEPTH, film=film)
    one = lambda lam: np.ones_like(np.asarray(lam, np.float64))
    w = sensor_white(film.imaging_ratio) if film.sensor == capi.RT_SENSOR_XYZ else \
        response(bars, film.imaging_ratio, one)
    o, d = camera_rays(cfg, _lattice())
    bq = d @ o
    disc = bq * bq - (o @ o - FURNACE_R ** 2)
    hit = disc > 0
    same = np.all(hit, axis=1) | ~np.any(hit, axis=1)
    on = np.all(hit, axis=1)
    include = same.copy()
    k = np.where(on, 0.9 if kind == "mirror" else 1.0, 1.0)
    if kind != "mirror":
        t = -bq - np.sqrt(np.maximum(disc, 0.0))
        x = o + t[..., None] * d
        cos_i = np.where(hit, -np.sum(x * d, axis=-1) / FURNACE_R, 1.0)
        etas = np.array([1.5]) if kind == "glass" else np.append(BK7_ETA[::5], BK7_ETA[-1])   # smooth in lambda
        f = fr_dielectric(cos_i[..., None], etas)
        lost = ((1 - f) * f ** (FURNACE_DEPTH - 1)).max(axis=(1, 2))
        include &= ~(on & (lost > LOST_MAX))
    mu = (l0 * k)[:, None] * w[None, :]
    if reflectance is not None:          # the sigmoid is at most 1: the white bound m8 holds on the sphere too
        wr = response(bars, film.imaging_ratio, lambda lam: sigmoid(reflectance, lam))
        mu = l0 * np.where(on[:, None], wr[None, :], w[None, :])
    vmax = l0 * (m1 if kind == "bk7" else m8) * (1 + 1e-5)
    return _finish(f"k6_furnace_{kind}", cfg, mu, vmax, include, spp)


# ------------------------------------------------------------------------------------------- reference integrator

AMBIENT = 0.3              # RT_INTEGRATOR_REFERENCE (include/rtmi355x.h): ambient 0.3 F1 + clamp(n.(0,0,-1)) D65 albedo
K_ILLUM = 2.0 * 0.5        # the light is RGBIlluminantSpectrum(sRGB, (1, 1, 1)): scale 2 max(rgb) times the sigmoid
                           # of rgb / scale = grey 0.5, times the colour space's illuminant D65
REF_FLIP_EPS = 1e-9
REF_EXPOSURE = 0.5


def kref_floor(albedo=0.5, spp=256, sensor="xyz", illum=capi.RT_ILLUM_D65):
    """The reference workload's own Li on the plain floor: L(lambda) = 0.3 F1(lambda) + c D65(round lambda) a, a the
    grey albedo_rgb.  F1 is a piecewise-linear table evaluated at the continuous wavelength, normalised as D65 is.
    c is the clamped dot of (0, 0, -1) with the mesh's OBJECT-space normal after it was flipped against the
    WORLD-space ray: with a normal (0, 0, +-1) it is 1 where the ray's z is positive and 0 where it is negative,
    whichever way the triangle is wound.  Pixels whose footprint holds both signs are excluded.
    This integrator has no light scale to choose, and F1's mercury lines at 405 and 436 nm lift one sample's Z to
    1.5 (albedo 0.5) and 1.75 (albedo 0.73) at the default imaging ratio, where it would clamp: the film's imaging
    ratio is halved (REF_EXPOSURE), which scales every expected value and bound alike."""
    model = _floor_model(False)
    cfg = _config("kref_floor", model, _down_camera(), spp, capi.RT_INTEGRATOR_REFERENCE, 1,
                  film=_film(sensor, illum, REF_EXPOSURE), albedo_rgb=(albedo,) * 3)
    nz = np.asarray(model.normals, np.float64)
    assert np.all(nz[:, :2] == 0) and np.all(np.abs(nz[:, 2]) == 1), "the floor's object-space normals are +-z"
    _floor_points(cfg, _lattice())                                  # every ray meets the floor
    _, d = camera_rays(cfg, _lattice())
    pos, neg = np.all(d[..., 2] > REF_FLIP_EPS, axis=1), np.all(d[..., 2] < -REF_FLIP_EPS, axis=1)
    c = pos.astype(np.float64)          # ray z > 0: the normal ends as (0, 0, -1) and the cosine is 1; else 0
    assert pos.mean() > 0.4 and neg.mean() > 0.4
    ir, bars = cfg.film.imaging_ratio, sensor_bars(cfg.film.sensor)
    a = float(sigmoid(scene.grey_sigmoid(albedo), 0.0))             # the constant sigmoid the descriptor's grey gives
    assert abs(a - albedo) < 1e-6
    f1 = illuminant(capi.RT_ILLUM_F1)
    ambient = AMBIENT * response(bars, ir, f1, table=np.ones(471))
    lit = K_ILLUM * a * response(bars, ir, lambda lam: np.ones_like(np.asarray(lam, np.float64)))
    mu = ambient[None, :] + c[:, None] * lit[None, :]
    # one sample is at most max over the scan of [0.3 F1(lambda) + a D65(round lambda)] bar / pdf: as an envelope of
    # the factor on D65(round lambda), 0.3 F1 / D65 + a, F1 taken over lambda +- 0.5 nm
    f1_env = bin_envelope(f1)
    env = lambda lam: AMBIENT * f1_env(lam) / D65[np.clip(np.rint(lam).astype(int) - 360, 0, 470)] + K_ILLUM * a
    m8, _ = sample_maxima(ir, bars=bars, envelope=env)
    return _finish("kref_floor", cfg, mu, m8, pos | neg, spp)


# ------------------------------------------------------------------------------------------- registry

# (id, builder, keyword arguments): every case and variant the CPU and GPU tests run.  `scene_key` groups the
# variants that share one uploaded scene.
CASES = [
    ("k1_point", k1_point, dict()),
    ("k1_point_tess", k1_point, dict(tessellated=True)),
    ("k1s_point_shadow", k1s_point_shadow, dict()),
    ("k2_distant", k2_distant, dict()),
    ("k3_quad_path_d1", k3_quad, dict(mis=False, max_depth=1)),
    ("k3_quad_path_d5", k3_quad, dict(mis=False, max_depth=5)),
    ("k3_quad_mis_d1", k3_quad, dict(mis=True, max_depth=1)),
    ("k3_quad_mis_d5", k3_quad, dict(mis=True, max_depth=5)),
    ("k3_quad_tess_path_d1", k3_quad, dict(mis=False, max_depth=1, tessellated=True)),
    ("k3_quad_tess_path_d5", k3_quad, dict(mis=False, max_depth=5, tessellated=True)),
    ("k3_quad_tess_mis_d1", k3_quad, dict(mis=True, max_depth=1, tessellated=True)),
    ("k3_quad_tess_mis_d5", k3_quad, dict(mis=True, max_depth=5, tessellated=True)),
    ("k3_quad_seen_path_d1", k3_quad, dict(mis=False, max_depth=1, seen=True)),
    ("k3_quad_seen_mis_d5", k3_quad, dict(mis=True, max_depth=5, seen=True)),
    ("k4_disk_path", k4_disk, dict(mis=False, max_depth=1)),
    ("k4_disk_mis", k4_disk, dict(mis=True, max_depth=2)),
    ("k5_sphere_d1", k5_sphere, dict(max_depth=1)),
    ("k5_sphere_d2", k5_sphere, dict(max_depth=2)),
    ("k5_sphere_d5", k5_sphere, dict(max_depth=5)),
    ("k6_furnace_mirror", k6_furnace, dict(kind="mirror")),
    ("k6_furnace_glass", k6_furnace, dict(kind="glass")),
    ("k6_furnace_bk7", k6_furnace, dict(kind="bk7")),
]

# The colour cases.  Variants of one scene are adjacent, and within a scene the sensor changes on its own at least
# once (k2: xyz -> canon -> sony; k3: the last two; k6; kref), so that a renderer reused across them must replace its
# sensor curves: a stale curve fails the closed form.
_A, _D50 = capi.RT_ILLUM_A, capi.RT_ILLUM_D50
_SENSOR_VARIANTS = [("xyz", "xyz", capi.RT_ILLUM_D65), ("canon", "canon_eos_100d", _A),
                    ("sony", "sony_ilce_6400", _D50)]
COLOUR_CASES = (
    [(f"k2_{cn}_{sn}", k2_distant, dict(albedo=c, sensor=sensor, illum=illum))
     for cn, c in (("red", S_RED), ("green", S_GREEN)) for sn, sensor, illum in _SENSOR_VARIANTS] +
    [("k1_red_tess", k1_point, dict(tessellated=True, albedo=S_RED)),
     ("k3_quad_green_path_d1", k3_quad, dict(mis=False, max_depth=1, albedo=S_GREEN)),
     ("k3_quad_green_mis_d5", k3_quad, dict(mis=True, max_depth=5, albedo=S_GREEN)),
     ("k3_quad_green_mis_d5_canon", k3_quad, dict(mis=True, max_depth=5, albedo=S_GREEN, sensor="canon_eos_100d",
                                                   illum=_A)),
     ("k5_red_d2", k5_sphere, dict(max_depth=2, albedo=S_RED)),
     ("k5_red_d5", k5_sphere, dict(max_depth=5, albedo=S_RED)),
     ("k5_green_d2", k5_sphere, dict(max_depth=2, albedo=S_GREEN)),
     ("k5_green_d5", k5_sphere, dict(max_depth=5, albedo=S_GREEN)),
     ("k6_furnace_mirror_red_xyz", k6_furnace, dict(kind="mirror", reflectance=S_RED)),
     ("k6_furnace_mirror_red_sony", k6_furnace, dict(kind="mirror", reflectance=S_RED, sensor="sony_ilce_6400",
                                                     illum=_D50)),
     ("kref_floor_a50", kref_floor, dict(albedo=0.5)),
     ("kref_floor_a73", kref_floor, dict(albedo=0.73)),
     ("kref_floor_a50_canon", kref_floor, dict(albedo=0.5, sensor="canon_eos_100d", illum=_A))])
CASES += COLOUR_CASES
CASE_IDS = [c[0] for c in CASES]


def scene_key(case_id):
    """Variants with the same key differ in the integrator descriptor and the film's sensor only."""
    for prefix in ("k3_quad_tess", "k3_quad_seen", "k3_quad_green", "k3_quad", "k4_disk", "k2_red", "k2_green",
                   "k5_red", "k5_green", "k6_furnace_mirror_red", "kref_floor"):
        if case_id.startswith(prefix):
            return prefix
    return case_id


_built = {}


def build_case(case_id):
    """(cfg, mu, vmax, include, spp) of a case, computed once and shared; callers must not modify the arrays."""
    if case_id not in _built:
        _, fn, kw = CASES[CASE_IDS.index(case_id)]
        cfg, mu, vmax, include = fn(**kw)
        for a in (mu, vmax, include):
            a.setflags(write=False)
        _built[case_id] = (cfg, mu, vmax, include, cfg.index_end - cfg.index_begin)
    return _built[case_id]
