"""CPU: albedo demodulation on its numpy restatement, tests/albedo_reference.py — the properties the
GPU kernels inherit by matching it bit for bit (tests/test_gpu_albedo.py), the quality statement on the oracle's films
of a textured floor against the float64 closed form, and the additive ABI."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import albedo_reference as aref
import denoise_reference as dref
import radiometry_reference as rref
import texture_reference as tref
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import ALBEDO_FLOOR_DEFAULT

ROOT = Path(__file__).resolve().parents[1]
F32 = np.float32
bits = dref.bits

FLOOR_COLOURS = np.array([(200, 60, 40), (40, 160, 90), (128, 128, 128), (50, 70, 220)], np.uint8)
# four greys or near-greys within +-24 codes of 128: texel contrast at or below the noise of a 16-spp film
LOW_CONTRAST = np.array([(128, 128, 128), (148, 148, 148), (108, 108, 108), (140, 126, 118)], np.uint8)
PALETTES = {"colours": FLOOR_COLOURS, "low_contrast": LOW_CONTRAST}
CAMERA_SENSOR = "canon_eos_100d"


# ------------------------------------------------------------------------------------------ 1. the sensor albedo
def test_dense_tables_equal_the_oracles(oracle_lib):
    """The float32 tables the restatement is evaluated on are the ones Spectra::Init builds."""
    got = [np.zeros(471, F32) for _ in range(4)]
    oracle_lib.lib().orc_spectra_dense(*(oracle_lib.fptr(a) for a in got))
    bars, d65 = aref.dense_tables("xyz")
    for a, b in zip(got, [bars[0], bars[1], bars[2], d65]):
        assert np.array_equal(bits(a), bits(b))
    cam, _ = aref.dense_tables(CAMERA_SENSOR)
    assert np.allclose(cam, rref.sensor_bars(CAMERA_SENSOR), rtol=1e-6, atol=1e-9)


def _inputs():
    return np.array([scene.grey_sigmoid(0.5), scene.grey_sigmoid(0.18), rref.S_RED, rref.S_GREEN] +
                    tref.rgb8_sigmoid(FLOOR_COLOURS).tolist(), F32)


@pytest.mark.parametrize("sensor", ["xyz", CAMERA_SENSOR])
def test_sensor_albedo_against_float64(sensor):
    """Relative error <= 1e-4: a 471-term sequential float32 sum of non-negative terms errs by at most about
    473 * 2^-24 = 2.8e-5 relative, in numerator and denominator alike, and the sigmoid adds a few ulp.

    Recorded (not asserted): the distance to response(bars, ir, sigmoid) / W, the bin-averaged expectation of the real
    estimator, which integrates the sigmoid over each 1 nm bin where the guide samples its centre: at most 3.7e-5
    relative (xyz) and 6.4e-5 (canon_eos_100d) over these inputs; the float32 sum itself is within 1.1e-6 and 3.4e-6
    of the float64 one."""
    bars, d65 = aref.dense_tables(sensor)
    assert np.all(bars >= 0) and np.all(d65 >= 0)
    co = _inputs()
    got = aref.sensor_albedo(co, bars, d65)
    want = aref.sensor_albedo64(co, bars, d65)
    rel = np.abs(got.astype(np.float64) - want) / want
    assert np.all(want > 0) and np.all(want < 1)
    assert rel.max() <= 1e-4, rel.max()
    b64 = rref.sensor_bars(sensor)
    dist = 0.0
    for c, w in zip(co, want):
        e = rref.response(b64, 1.0, lambda lam: rref.sigmoid(c, lam)) / (b64 @ rref.D65)
        dist = max(dist, float(np.max(np.abs(w - e) / e)))
    print(f"{sensor}: float32 vs float64 {rel.max():.3e}; float64 sum vs the estimator's expectation {dist:.3e}")


def test_sensor_albedo_limits():
    bars, d65 = aref.dense_tables("xyz")
    co = np.array([(0, 0, 0), (0, 0, np.inf), (0, 0, -np.inf), (0, 0, 1e30), (0, 0, -1e30)], F32)
    a = aref.sensor_albedo(co, bars, d65)
    assert np.all(a[0] == F32(0.5)) or np.allclose(a[0], 0.5, rtol=1e-6)
    assert np.allclose(a[1], 1.0, rtol=1e-6) and np.all(a[2] == 0)
    assert np.allclose(a[3], 0.5, rtol=1e-6)           # x x overflows: x / inf = 0, as the kernel computes it
    assert np.all(np.isfinite(a))


# ------------------------------------------------------------------------------------------ 2. the filter
def _synthetic(W, H, seed):
    """test_gpu_denoise.synthetic's kind of input, smaller: noisy film, moments, two normals and a depth ramp."""
    rng = np.random.default_rng(seed)
    N = W * H
    y, x = np.divmod(np.arange(N), W)
    nrm = np.where((x < W // 2)[:, None], [0.0, 0.0, -1.0], [0.6, 0.0, -0.8])
    feat = (np.concatenate([nrm, (500.0 + 3.0 * x + 1.5 * y)[:, None]], axis=1) * 4).astype(F32)
    n = rng.integers(2, 40, N).astype(F32)
    n[rng.random(N) < 0.05] = 0
    a = np.abs(0.5 + rng.normal(0, 0.1, (N, 3))).astype(F32)
    film = np.concatenate([a * n[:, None], n[:, None]], axis=1).astype(F32)
    s = (film[:, 0] + film[:, 1]) + film[:, 2]
    with np.errstate(all="ignore"):
        q = np.where(n > 0, s.astype(np.float64) ** 2 / np.maximum(n, 1) + n * rng.uniform(0.01, 0.4, N) ** 2, 0.0)
    return film, np.stack([s, q], axis=1).astype(F32), feat


@pytest.mark.parametrize("k", [1.0, 4.0, 0.375])
def test_constant_albedo_film_equals_the_plain_filter(k):
    """An albedo film of all (k, k, k, k) is a = (1, 1, 1), sa = 1: dividing and multiplying by 1 are exact."""
    W, H = 37, 29
    film, mom, feat = _synthetic(W, H, 3)
    alb = np.full((W * H, 4), k, F32)
    for it in (1, 5):
        p = dict(dref.DEFAULTS, iterations=it)
        want, want_var = dref.denoise(film, mom, feat, W, H, **p)
        out, var = aref.denoise_albedo(film, mom, feat, alb, W, H, ALBEDO_FLOOR_DEFAULT, **p)
        assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(var), bits(want_var))
    # pixels without a hit are not demodulated either
    alb[::3] = 0
    out, _ = aref.denoise_albedo(film, mom, feat, alb, W, H, ALBEDO_FLOOR_DEFAULT, **dref.DEFAULTS)
    assert np.array_equal(bits(out), bits(dref.denoise(film, mom, feat, W, H, **dref.DEFAULTS)[0]))


def test_constant_irradiance_returns_the_texture():
    """film = (a i) n with i constant and a a random texture above the floor: out / n equals a i within 264 u relative,
    u = 2^-24 one rounding, 1.6e-5, where the plain filter is off by more than 5 %.

    The bound, to first order in u, per channel.  n = 16 is a power of two, so multiplying and dividing by n are
    exact.  The film holds fl(a i) n = a i (1 + e1) n; prepare's c = (f / n) / a = i (1 + e), |e| <= 2 u (the product's
    rounding and the one division).  An iteration returns sr / sw over at most 25 taps with weights w >= 0 summed in
    the same order: fl(sr) = sum w_q c_q (1 + d_q), |d_q| <= 26 u (a product and at most 25 additions), fl(sw) =
    sum w_q (1 + d'_q), |d'_q| <= 25 u, and the division rounds once, so inputs within i (1 +- E) come out within
    i (1 +- (E + 52 u)).  Five iterations: 2 u + 5 * 52 u = 262 u.  The finish rounds once per channel (c' a; times n
    is exact), and the float64 reference a i takes the float32 a and i exactly: 263 u, asserted as 264 u."""
    W, H = 40, 24
    rng = np.random.default_rng(11)
    N = W * H
    a = rng.uniform(0.1, 0.95, (N, 3)).astype(F32)
    i = F32(0.7)
    n = F32(16)
    film = np.concatenate([(a * i) * n, np.full((N, 1), n, F32)], axis=1).astype(F32)
    s = (film[:, 0] + film[:, 1]) + film[:, 2]
    mom = np.stack([s, s * s / n + F32(0.5)], axis=1).astype(F32)      # some variance: the luminance stop is open
    feat = np.zeros((N, 4), F32)
    feat[:, 2], feat[:, 3] = -4, 4 * 500
    alb = np.concatenate([a * F32(4), np.full((N, 1), 4, F32)], axis=1).astype(F32)   # 4 hits of albedo a: exact
    out, _ = aref.denoise_albedo(film, mom, feat, alb, W, H, ALBEDO_FLOOR_DEFAULT, **dref.DEFAULTS)
    want = a.astype(np.float64) * float(i)
    rel = np.abs(out[:, :3].astype(np.float64) / float(n) - want) / want
    u = 2.0 ** -24
    print(f"largest relative error {rel.max() / u:.2f} u")
    assert rel.max() <= 264 * u, rel.max() / u
    # the plain filter blurs the same film: it is not the texture any more
    plain, _ = dref.denoise(film, mom, feat, W, H, **dref.DEFAULTS)
    assert (np.abs(plain[:, :3].astype(np.float64) / float(n) - want) / want).max() > 0.05


# ------------------------------------------------------------------------------------------ 3. quality on the oracle
def floor_cfg(tessellated, palette=None):
    """The floor scene of tests/test_gpu_texture.py: 64x64, the camera straight down on the floor y = 0, a distant
    light, max_depth 1, 4x4 stratified samples; with `palette` a 16x16 texture of its four colours whose texels cover
    4x4 pixels each.  Returns (cfg, colour index per pixel or None)."""
    lights = [dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(rref.K2_DIR), scale=rref.K2_E)]
    cfg = scene.Config("floor", rref._floor_model(tessellated, lights=lights), rref._down_camera(),
                       scene.StratifiedSampler(4, 4, False, 0), scene.Film(res=rref.RES),
                       scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=1), 0, 16)
    if palette is None:
        return cfg, None
    pat = np.random.default_rng(13).integers(0, 4, (16, 16))
    lat = rref._floor_points(cfg, np.array([[0.0, 0.0], [1.0, 1.0]]))
    x0, x1, z0, z1 = lat[..., 0].min(), lat[..., 0].max(), lat[..., 2].min(), lat[..., 2].max()
    m = cfg.model
    pos = np.asarray(m.positions, np.float64)
    m.texcoords = np.stack([(pos[:, 0] - x0) / (x1 - x0), (pos[:, 1] - z0) / (z1 - z0)], -1).astype(F32)
    m.textures = [scene.Texture(np.asarray(palette, np.uint8)[pat], wrap="clamp")]
    m.material_texture = [0]
    pts = rref._floor_points(cfg, rref._midpoints(4))
    tu, tv = (pts[..., 0] - x0) / (x1 - x0) * 16, (pts[..., 2] - z0) / (z1 - z0) * 16
    ix, iy = np.floor(tu).astype(int), np.floor(tv).astype(int)
    assert np.all(ix == ix[:, :1]) and np.all(iy == iy[:, :1]), "a pixel's samples share one texel"
    return cfg, pat[iy[:, 0], ix[:, 0]]


def floor_truth(cfg, palette, colour):
    """The float64 closed form per pixel: K2_GEOMETRY * response(BARS, imaging_ratio, sigmoid(texel coefficients))."""
    co = tref.rgb8_sigmoid(np.asarray(palette, np.uint8))
    per = np.stack([rref.K2_GEOMETRY * rref.response(rref.BARS, cfg.film.imaging_ratio,
                                                     lambda lam, c=c: rref.sigmoid(c, lam)) for c in co])
    return per[colour]


def mse(film, truth):
    return float(np.mean((film[:, :3].astype(np.float64) / film[:, 3:4] - truth) ** 2))


def flip_x(a, W, H):
    return np.ascontiguousarray(a.reshape(H, W, -1)[:, ::-1]).reshape(W * H, -1)


def quality_arms(film, mom, feat, alb, truth, W, H, albedo_floor=ALBEDO_FLOOR_DEFAULT, denoise=None, denoise_albedo=None):
    """MSE of the unfiltered film, the plain filter, the demodulating filter and the demodulating filter with the albedo
    film flipped in x, by the numpy references or the given callables."""
    denoise = denoise or (lambda f, m, g: dref.denoise(f, m, g, W, H, **dref.DEFAULTS)[0])
    denoise_albedo = denoise_albedo or (lambda f, m, g, a: aref.denoise_albedo(f, m, g, a, W, H, albedo_floor,
                                                                              **dref.DEFAULTS)[0])
    return dict(unfiltered=mse(film, truth), plain=mse(denoise(film, mom, feat), truth),
                demodulated=mse(denoise_albedo(film, mom, feat, alb), truth),
                flipped=mse(denoise_albedo(film, mom, feat, flip_x(alb, W, H)), truth))


@pytest.fixture(scope="module")
def oracle_floor(oracle_lib):
    """Per palette: the oracle's 16-spp film and moments of the textured floor (composed per pixel from its films of
    the four uniformly coloured floors, as tests/test_gpu_texture.py does), the feature and albedo films of indices
    [0, 4) from its sample records, and the closed form."""
    W, H = rref.RES
    out = {}
    bars, d65 = aref.dense_tables("xyz")
    for name, pal in PALETTES.items():
        cfg, colour = floor_cfg(False, pal)
        film, mom = np.zeros((W * H, 4), F32), np.zeros((W * H, 2), F32)
        scenes = []
        for c in pal:
            u, _ = floor_cfg(False)
            u.model = rref._floor_model(False, lights=u.model.lights,
                                        albedo=scene.rgb_albedo(tuple(tref.rgb8_to_float(c).tolist())))
            scenes.append(oracle_lib.OracleScene(u))
        for i in range(16):
            one = np.zeros((W * H, 4), F32)
            for k, o in enumerate(scenes):
                one[colour == k] = o.render(i, i + 1)[colour == k]
            film = film + one
            v = (one[:, 0] + one[:, 1]) + one[:, 2]
            mom[:, 0] = mom[:, 0] + v
            mom[:, 1] = mom[:, 1] + v * v
        rc = dref.record_config(cfg)
        o = oracle_lib.OracleScene(rc)
        feat = dref.oracle_features(o, dref.world_triangles(rc.model), W, H, 0, 4)
        alb = aref.oracle_albedo(o, cfg, W, H, 0, 4, bars, d65)
        out[name] = dict(film=film, mom=mom, feat=feat, alb=alb, truth=floor_truth(cfg, pal, colour))
    return out


def test_quality_on_the_oracles_textured_floor(oracle_floor):
    """64x64 floor, 16x16 texture of 4x4-pixel texels, 16 spp, every input from the oracle, MSE of the mean colour
    against the float64 closed form (DESIGN.md §3h has the table)."""
    W, H = rref.RES
    rows = {}
    for name, d in oracle_floor.items():
        assert np.all(d["alb"][:, 3] == 4) and np.all(d["film"][:, 3] == 16)
        rows[name] = quality_arms(d["film"], d["mom"], d["feat"], d["alb"], d["truth"], W, H)
        print(name, {k: f"{v:.4e}" for k, v in rows[name].items()})
    for name, r in rows.items():
        assert r["demodulated"] < r["unfiltered"], name
        assert r["flipped"] > r["demodulated"], name      # the power test: a wrong albedo film does not pass
    assert rows["low_contrast"]["demodulated"] < rows["low_contrast"]["plain"]


def test_albedo_floor_default(oracle_floor):
    """ALBEDO_FLOOR_DEFAULT is the candidate of {1/256, 1/64, 1/16} with the lowest MSE on the FLOOR_COLOURS floor at
    16 spp (DESIGN.md §3h has the table); ties go to the smallest floor, which alters the fewest albedos."""
    W, H = rref.RES
    d = oracle_floor["colours"]
    got = {}
    for af in (1 / 256, 1 / 64, 1 / 16):
        out, _ = aref.denoise_albedo(d["film"], d["mom"], d["feat"], d["alb"], W, H, af, **dref.DEFAULTS)
        got[af] = mse(out, d["truth"])
        print(f"albedo_floor 1/{round(1 / af)}: MSE {got[af]:.4e}")
    best = min(got, key=lambda k: (got[k], k))
    assert ALBEDO_FLOOR_DEFAULT == best, got


# ------------------------------------------------------------------------------------------ 4. the ABI
NEW_SYMBOLS = ["rt_render_features_albedo", "rt_denoise_albedo", "rt_adaptive_denoise_albedo", "rt_debug_albedo_bake"]


def test_exports_and_struct_size(tmp_path):
    text = (ROOT / "include" / "rtmi355x.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(rt_\w+)\s*\(", text, re.M))
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in capi.EXPORTS, s
        f = getattr(lib, s)
        assert f.restype is C.c_int and f.argtypes, s
    assert C.sizeof(capi.rt_albedo) == 16
    assert [f for f, _ in capi.rt_albedo._fields_] == ["r", "g", "b", "hits"]
    assert lib.rt_abi_version() == 10
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "rtmi355x.h"\nint main(void) { printf("%zu\\n", sizeof(rt_albedo)); '
                   'return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == ["16"]
    # host-only behaviour: a NULL context is RT_E_ARG, never a crash
    assert lib.rt_render_features_albedo(None, 0, 1, 0, None, None, None) == capi.RT_E_ARG
    assert lib.rt_denoise_albedo(None, None, 0.1, 1, 1, None, None, None, None, None, None) == capi.RT_E_ARG
    assert lib.rt_adaptive_denoise_albedo(None, None, 0.1, None) == capi.RT_E_ARG
    assert lib.rt_debug_albedo_bake(None, 0, None, None) == capi.RT_E_ARG
