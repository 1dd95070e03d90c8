"""The image environment light (RT_LIGHT_ENV) on the device: the bake's table, the sampling and the
miss stage's lookup bit for bit against tests/envlight_reference.py, films against float64 closed forms, and
rt_scene_set_environment's validation.  The oracle cannot render an environment, so nothing here compares with it."""
import ctypes as C

import numpy as np
import pytest

import envlight_reference as er
import radiometry_reference as ref
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
f32 = np.float32
ROT = er.colmajor(er.E2_M)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def floor():
    """One context over the plain floor (PATH depth 1, 16 spp): the table, sampling and validation tests bind maps to it."""
    cfg = ref._config("env_floor", ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,
                      film=ref._film())
    g = Renderer(cfg)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------ 1. bake and table

@pytest.mark.parametrize("name", er.TABLE_MAPS)
def test_table_bit_for_bit(floor, name):
    rgb = er.table_map(name)
    H, W = rgb.shape[:2]
    floor.set_environment(scene.Environment(rgb, scale=1.5, world_to_env=er.E2_M))
    t = floor.env_table()
    m, w = er.bake_weights(rgb)
    cond, marg, total = er.table(w)
    assert t["cond"].shape == (H, W) and t["marg"].shape == (H,)
    assert np.array_equal(bits(t["coeffs"][..., 3]), bits(m)), "m = 2 max(r, g, b)"
    assert np.array_equal(bits(t["cond"]), bits(cond)), f"{np.sum(bits(t['cond']) != bits(cond))} conditional entries differ"
    assert np.array_equal(bits(t["marg"]), bits(marg)), f"{np.sum(bits(t['marg']) != bits(marg))} marginal entries differ"
    assert bits(t["total"]) == bits(total) and t["marg"][-1] == f32(1.0)
    # the coefficients: rt_rgb_to_sigmoid(rgb / m) per texel, all 0 for a black texel
    lib = floor.lib
    flat, co = rgb.reshape(-1, 3), t["coeffs"].reshape(-1, 4)
    idx = np.unique(np.concatenate([np.arange(min(64, len(flat))), np.flatnonzero(m.reshape(-1) == 0)[:8]]))
    for i in idx:
        if m.reshape(-1)[i] == 0:
            assert np.all(co[i] == 0)
            continue
        q = (flat[i] / m.reshape(-1)[i]).astype(f32)
        out = np.zeros(3, f32)
        assert lib.rt_rgb_to_sigmoid(q.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert np.array_equal(bits(co[i, :3]), bits(out)), i
    if name == "black":
        assert np.all(t["cond"][5] == 0) and t["marg"][5] == t["marg"][4], "the black row: zero marginal step"
        # (behind the black half a row's sums repeat up to the scan's ulp dips, DESIGN.md §3i: no exact plateau)
        assert np.all(np.abs(t["cond"][:, 19:][np.arange(12) != 5] - 1) <= 2.0 ** -22)


# ------------------------------------------------------------------------------------------ 2. sampling, evaluation

@pytest.mark.parametrize("name", er.TABLE_MAPS)
def test_sample_and_eval_bit_for_bit(floor, name):
    rgb = er.table_map(name)
    H, W = rgb.shape[:2]
    floor.set_environment(scene.Environment(rgb, world_to_env=er.E2_M))
    _, w = er.bake_weights(rgb)
    cond, marg, _ = er.table(w)
    u = er.sample_points(cond, marg)
    assert len(u) == 4096
    want = er.sample(cond, marg, ROT, u)
    got = floor.env_sample(u)
    assert np.array_equal(got["texel"], want["texel"]), f"{np.sum(got['texel'] != want['texel'])} texels differ"
    assert np.array_equal(bits(got["wi"]), bits(want["wi"])), f"{np.sum(bits(got['wi']) != bits(want['wi']))} wi values differ"
    assert np.array_equal(bits(got["pdf"]), bits(want["pdf"])), f"{np.sum(bits(got['pdf']) != bits(want['pdf']))} pdfs differ"
    ok = want["pdf"] > 0
    # behind black texels the scan's sums can rise by an ulp as well as dip, which gives a black texel a
    # step of that size: a sample there is accepted with that pdf and adds Le = 0.  Rare, and only at such steps.
    stray = ok & (w.reshape(-1)[want["texel"]] == 0)
    assert stray.mean() < 2e-3 and np.all(er.bake_weights(rgb)[0].reshape(-1)[want["texel"][stray]] == 0)
    # evaluation: random directions and the sampled ones
    rng = np.random.default_rng(4)
    d = np.concatenate([rng.normal(size=(2048, 3)).astype(f32), want["wi"][:2048]])
    e_want = er.evaluate(cond, marg, ROT, d)
    e_got = floor.env_eval(d)
    assert np.array_equal(e_got["texel"], e_want["texel"])
    assert np.array_equal(bits(e_got["pdf"]), bits(e_want["pdf"]))
    # round trip: the miss stage finds the sampled texel and its pdf, except within 1e-3 texel of a border
    back = floor.env_eval(got["wi"])
    inner = ok & (er.border_distance(want["s"], want["t"], W, H) >= 1e-3)
    excluded = 1.0 - inner[ok].mean() if ok.any() else 0.0
    print(f"{name}: {excluded:.4f} of the accepted samples lie within 1e-3 texel of a border")
    assert excluded < 0.02
    assert np.array_equal(back["texel"][inner], got["texel"][inner])
    assert np.allclose(back["pdf"][inner], got["pdf"][inner], rtol=2e-5)    # |p|^3 through one float32 round trip


# ------------------------------------------------------------------------------------------ 3. films

def _film(cfg, env, spp):
    g = Renderer(cfg)
    try:
        g.set_environment(env)
        oc = g.octree()
        depth = oc["depth"], oc["max_queue_groups"]
        g.reset_stats()
        film = g.render_pass(0, spp)
        return film, g.stats(), depth, g.env_miss_ms()
    finally:
        g.close()


def _closed_form(name, case, spp=256, multi_level=None):
    cfg, env, mu, vmax, include = case
    film, st, depth, ms_miss = _film(cfg, env, spp)
    if multi_level is not None:
        assert depth[0] > 0 if multi_level else depth[0] == 0
        assert (depth[1] > 16) == multi_level, depth   # (QCAP 0 with coop_ok: DESIGN §2)
    assert st["coop_overflows"] == 0 and ms_miss > 0, "the miss stage ran"
    rows = ref.compare(film, mu, vmax, include, spp)
    print(f"{name}: max |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), ref.report(rows)
    for factor in (1.03, 0.97):                      # and it would not pass with a 3 % error
        assert not ref.passes(ref.compare(film, factor * mu, vmax, include, spp))
    return film, st


@pytest.mark.parametrize("tessellated", [False, True], ids=["plain", "tessellated"])
@pytest.mark.parametrize("mis,depth,res_map", [(False, 1, (1, 1)), (True, 1, (8, 4)), (True, 5, (1, 1))],
                         ids=["path1", "mis1", "mis5"])
def test_e1_constant_map_over_the_floor(mis, depth, res_map, tessellated):
    """floor = rho c response(1) at every depth; under MIS the NEE and the miss weights sum to one."""
    _, st = _closed_form(f"e1 mis={mis} depth={depth} map={res_map} tess={tessellated}",
                         er.e1(mis, depth, tessellated, res_map), multi_level=tessellated)
    assert st["nee_vertices"] > 0


def test_e1_sky_pixels():
    """Camera rays that leave the scene: every pixel = c response(1) (k_env_miss at depth 0, prevPdf == 0)."""
    _, st = _closed_form("e1 sky", er.sky_case())
    assert st["nee_vertices"] == 0 and st["hits"] == 0


@pytest.mark.parametrize("mis", [False, True], ids=["path", "mis"])
def test_e2_bright_patch_rotated(mis):
    _closed_form(f"e2 mis={mis}", er.e2(mis, 1))


def test_e3_disk_shadow():
    """The only occluder between a shading point and the map: environment shadow rays (tmax = FLT_MAX) against an
    analytic shape.  Pixels whose whole view of the patch is blocked are exactly 0."""
    case = er.e3()
    cfg, env, mu, vmax, include = case
    umbra = include & np.all(mu == 0, axis=1)
    print(f"e3: {umbra.sum()} umbra pixels, {(include & ~umbra).sum()} lit, {1 - include.mean():.3f} excluded (penumbra, rim)")
    film, st = _closed_form("e3", case)
    img = film[:, :3] / film[:, 3:4]
    assert np.all(img[umbra] == 0) and st["shadow_rays"] > 0
    # without the occluder the same pixels are lit: the zeros are the disk's doing
    open_cfg = er.e3()[0]
    open_cfg.model.shapes = []
    bare, _, _, _ = _film(open_cfg, env, 256)
    assert np.all((bare[:, :3] / bare[:, 3:4])[umbra].mean(axis=0) > 0.5 * mu[include & ~umbra].mean(axis=0))


@pytest.mark.parametrize("kind,depth,mis", [("lambert", 1, False), ("lambert", 5, False), ("lambert", 5, True),
                                            ("mirror", 0, False), ("glass", 0, False)],
                         ids=["lambert1", "lambert5", "lambert5mis", "mirror", "glass"])
def test_e4_sphere_under_a_constant_map(kind, depth, mis):
    """An analytic shape: NEE from a sphere, a miss after a specular bounce (prevPdf == 0), the sky beside it."""
    _closed_form(f"e4 {kind} depth={depth} mis={mis}", er.e4(kind, depth, mis))


@pytest.mark.parametrize("sensor", ["xyz", "canon_eos_100d"])
@pytest.mark.parametrize("sky", [False, True], ids=["floor", "sky"])
def test_e5_coloured_map(floor, sensor, sky):
    """Per-wavelength Le in k_path_nee (floor) and k_env_miss (sky), on the XYZ sensor and a camera's curves."""
    floor.set_environment(er.e5_env())
    co = floor.env_table()["coeffs"]
    assert np.all(co == co[0, 0]) and co[0, 0, 3] == f32(2 * 0.63)
    _closed_form(f"e5 {sensor} sky={sky}", er.e5(co[0, 0], sensor, sky))


@pytest.mark.parametrize("tessellated", [False, True], ids=["plain", "tessellated"])
def test_e7_textured_floor(floor, tessellated):
    """An albedo texture on the floor under the map: the TEX and the environment instantiations together."""
    co = floor.texture_bake(np.full((1, 3), er.E7_GREY, np.uint8))[0]
    _, st = _closed_form(f"e7 tess={tessellated}", er.e7(co, tessellated), multi_level=tessellated)
    assert st["nee_vertices"] > 0


def test_e6_quad_light_plus_dim_map():
    """K3's quad light first, the map second: nee_stride with two lights, both closed forms summed."""
    _closed_form("e6", er.e6())


# ------------------------------------------------------------------------------------------ 4. binding

def test_without_a_map_nothing_changes_and_clearing_restores_the_film():
    cfg = ref.k2_distant(spp=16)[0]
    g = Renderer(cfg)
    try:
        g.reset_stats()
        n0 = g.tabled_launches()
        before = g.render_pass(0, 16)
        assert g.env_miss_ms() == 0 and before[:, :3].max() > 0
        n1 = g.tabled_launches()       # the kernels that ran: the old instantiations (TL = 0) alone
        for k in ("shade", "nee"):
            assert (n1[k] - n0[k])[0] > 0 and np.all((n1[k] - n0[k])[1:] == 0), (k, n1[k] - n0[k])
        g.set_environment(scene.Environment(er.constant_map(8, 4, (0.02,) * 3)))
        g.reset_stats()
        lit = g.render_pass(0, 16)
        assert g.env_miss_ms() > 0 and g.stats()["nee_vertices"] > 0
        n2 = g.tabled_launches()       # ... with a map: the environment instantiations (TL = 2) alone
        for k in ("shade", "nee"):
            assert (n2[k] - n1[k])[2] > 0 and np.all((n2[k] - n1[k])[:2] == 0), (k, n2[k] - n1[k])
        assert lit[:, :3].sum() > before[:, :3].sum()
        # a split pass accumulates to the same bits
        split = g.render_pass(0, 5)
        split = g.render_pass(5, 16, split)
        assert np.array_equal(bits(split), bits(lit))
        g.set_environment(None)
        g.reset_stats()
        n3 = g.tabled_launches()
        after = g.render_pass(0, 16)
        assert g.env_miss_ms() == 0
        n4 = g.tabled_launches()       # ... and the old ones again
        for k in ("shade", "nee"):
            assert (n4[k] - n3[k])[0] > 0 and np.all((n4[k] - n3[k])[1:] == 0), (k, n4[k] - n3[k])
        assert np.array_equal(bits(after), bits(before)), "clearing the map gives back the pre-map film"
        # a new upload drops the map
        g.set_environment(scene.Environment(er.constant_map(2, 2, (0.02,) * 3)))
        g.configure(cfg)
        with pytest.raises(capi.RTError):
            g.env_table()
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(before))
    finally:
        g.close()


def test_missing_coefficient_table_is_a_state_error(tmp_path):
    """The table is loaded once per process, so this runs in a fresh one with RTMI_RGBSPEC_TABLE pointing nowhere."""
    import os
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    code = ("import sys, ctypes as C\n"
            f"sys.path.insert(0, {str(root)!r}); sys.path.insert(0, {str(root / 'tests')!r})\n"
            "import numpy as np\n"
            "import radiometry_reference as ref\n"
            "from computational_ray_tracer_amd import capi, scene\n"
            "from computational_ray_tracer_amd.renderer import Renderer\n"
            "cfg = ref._config('env_floor', ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,\n"
            "                  film=ref._film())\n"                    # (a grey floor: building it needs no table)
            "g = Renderer(cfg)\n"
            "d = scene.Environment(np.full((2, 4, 3), 0.1, np.float32)).desc()\n"
            "rc = g.lib.rt_scene_set_environment(g.h, C.byref(d))\n"
            "print('RC', rc, g.lib.rt_last_error(g.h).decode())\n"
            "g.close()\n")
    env = dict(os.environ, RTMI_RGBSPEC_TABLE=str(tmp_path / "missing.rgbspec"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("RC")][0]
    assert line.split()[1] == str(capi.RT_E_STATE) and "table" in line, line


def test_validation(floor):
    g = floor
    good_env = scene.Environment(er.constant_map(4, 2, (0.05,) * 3))
    g.set_environment(good_env)
    good = g.render_pass(0, 16)
    assert good[:, :3].max() > 0

    def call(mutate):
        d = good_env.desc()
        mutate(d)
        rc = g.lib.rt_scene_set_environment(g.h, C.byref(d))
        return rc, g.lib.rt_last_error(g.h).decode()

    def bad(mutate, code=capi.RT_E_ARG):
        rc, msg = call(mutate)
        assert rc == code and msg, (capi.STATUS_NAMES.get(rc, rc), msg)
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(good)), "a rejected call changes nothing"

    bad(lambda d: setattr(d, "width", -1))
    bad(lambda d: setattr(d, "height", 0))
    bad(lambda d: setattr(d, "rgb", None))
    bad(lambda d: setattr(d, "scale", -1.0))
    bad(lambda d: setattr(d, "scale", float("nan")))

    def texel(v):
        def f(d):
            d._rgb[0, 1, 2] = v
        return f
    bad(texel(-1e-3))
    bad(texel(float("inf")))
    bad(texel(float("nan")))

    def black(d):
        d._rgb[:] = 0
    bad(black)                                       # a zero total

    def huge(d):
        d.width, d.height = 1 << 13, (1 << 11) + 1   # (validated before the texels are read)
    bad(huge, capi.RT_E_LIMIT)
    rc, msg = call(lambda d: None)
    assert rc == capi.RT_OK, msg
    # RT_E_STATE: no scene; an open adaptive session
    h = Renderer()
    try:
        d = good_env.desc()
        assert h.lib.rt_scene_set_environment(h.h, C.byref(d)) == capi.RT_E_STATE
    finally:
        h.close()
    ad = capi.rt_adaptive_desc(min_samples=2, step_samples=2, max_samples=4, rel_error=0.1, abs_floor=0.0)
    assert g.lib.rt_adaptive_begin(g.h, C.byref(ad)) == capi.RT_OK
    try:
        d = good_env.desc()
        assert g.lib.rt_scene_set_environment(g.h, C.byref(d)) == capi.RT_E_STATE
        assert g.lib.rt_scene_set_environment(g.h, None) == capi.RT_E_STATE
    finally:
        assert g.lib.rt_adaptive_end(g.h) == capi.RT_OK
    # ... an open temporal session
    g.temporal_begin()
    try:
        d = good_env.desc()
        assert g.lib.rt_scene_set_environment(g.h, C.byref(d)) == capi.RT_E_STATE
        assert "temporal" in g.lib.rt_last_error(g.h).decode()
    finally:
        g.temporal_end()
    assert np.array_equal(bits(g.render_pass(0, 16)), bits(good))
    # RT_LIGHT_ENV is the device's type only: rt_scene_upload rejects it in a light list and keeps the scene and the map
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_ENV, scale=1.0)])
    sd = m.desc()
    assert g.lib.rt_scene_upload(g.h, C.byref(sd)) == capi.RT_E_ARG
    assert "light type" in g.lib.rt_last_error(g.h).decode()
    assert np.array_equal(bits(g.render_pass(0, 16)), bits(good))
    # a full light list
    lights = [dict(type=capi.RT_LIGHT_POINT, p=(0.0, 500.0 + i, 0.0), scale=1.0) for i in range(64)]
    cfg = ref._config("env_full", ref._floor_model(False, lights=lights), ref._down_camera(), 16,
                      capi.RT_INTEGRATOR_PATH, 1, film=ref._film())
    f = Renderer(cfg)
    try:
        d = good_env.desc()
        assert f.lib.rt_scene_set_environment(f.h, C.byref(d)) == capi.RT_E_ARG
        assert "light" in f.lib.rt_last_error(f.h).decode()
    finally:
        f.close()
    g.set_environment(None)
