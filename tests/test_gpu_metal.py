"""The metals (RT_MAT_CONDUCTOR) on the device: the level-2 kernels' device functions bit for bit against
tests/metal_reference.py, rt_scene_upload's and rt_scene_set_textures' validation, which instantiations a scene runs, split
passes, and films against float64 closed forms.  The oracle does not know this material: nothing here renders through it.

Film cases: M1 (distant light over a gold floor, alpha 0.5 and 0.2, single-leaf and multi-level), M1g (the same floor seen
and lit at grazing angles), M2 (quad light over copper, PATH and PATH_MIS), M3 (a gold sphere under a constant map: PATH
depth 1, PATH_MIS depth 1 and 5), M4 (the floor seen in a mirror wall), M5 (half the floor rough grey), M6 (aluminium on the
Sony sensor).  The measured |got - mu| / tol of each is recorded in DESIGN.md §3l.
"""
import ctypes as C

import numpy as np
import pytest

import metal_reference as mr
import radiometry_reference as ref
import rough_reference as rr
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
f32 = np.float32
SPP = 256


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def floor():
    """One context over the plain Lambert floor: the debug entry uses it."""
    cfg = ref._config("metal_floor", ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,
                      film=ref._film())
    g = Renderer(cfg)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------ 1. the device functions

def _debug_inputs(n=4096, seed=9):
    """Unit normals all over the sphere, incoming directions from grazing to head-on, light directions of which an eighth
    of those below the horizon stay there, wavelengths over 355..835 with both table edges and some x.5 among them."""
    rng = np.random.default_rng(seed)
    nrm = rr.nrm64(rng.normal(size=(n, 3)))
    nrm[:4] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]]
    t = rr.nrm64(np.cross(nrm, rng.normal(size=(n, 3))))
    mu = np.concatenate([np.full(64, 1e-3), np.geomspace(1e-3, 1.0, 512), rng.random(n - 64 - 512 - 64), np.full(64, 1.0)])
    d = -(mu[:, None] * nrm + np.sqrt(1 - mu * mu)[:, None] * t)
    wi = rr.nrm64(rng.normal(size=(n, 3)))
    flip = np.sum(wi * nrm, -1) < 0
    wi[flip & (np.arange(n) % 8 != 0)] *= -1
    wi[64:128] = -d[64:128]                                   # wi = wo: wo.h = 1 whatever mu_o is
    lam = (355 + 480 * rng.random(n)).astype(f32)
    lam[:8] = [359.4, 359.5, 830.49, 830.5, 449.5, 450.49, 360.0, 830.0]
    as32 = lambda a: rr.norm32(a.astype(f32))
    return as32(nrm), as32(d), as32(wi), lam


@pytest.mark.parametrize("metal", range(4))
@pytest.mark.parametrize("alpha", [0.01, 0.2, 1.0])
def test_device_functions_bit_for_bit(floor, alpha, metal):
    nrm, d, wi, lam = _debug_inputs()
    got = floor.conductor_eval(metal, alpha, nrm, d, wi, lam)
    fc, pdf, F = mr.debug_eval32(mr.METALS[metal], alpha, nrm, d, wi, lam)
    assert (fc == 0).sum() > 100 and (fc > 0).sum() > 2000
    assert np.array_equal(bits(got["fcos"]), bits(fc)), f"{np.sum(bits(got['fcos']) != bits(fc))} fcos differ"
    assert np.array_equal(bits(got["pdf"]), bits(pdf)), f"{np.sum(bits(got['pdf']) != bits(pdf))} pdfs differ"
    ok = ~np.isnan(F)                                          # (outside 360-830: n = k = 0, where F may be 0 / 0)
    assert ok.sum() > 4000 and np.array_equal(np.isnan(got["F"]), ~ok)
    assert np.array_equal(bits(got["F"][ok]), bits(F[ok])), f"{np.sum(bits(got['F'][ok]) != bits(F[ok]))} F differ"
    # fcos and pdf have rt_debug_ggx_eval's bits on the same inputs
    ev = floor.ggx_eval(alpha, nrm, d, wi)
    assert np.array_equal(bits(got["fcos"]), bits(ev["fcos"])) and np.array_equal(bits(got["pdf"]), bits(ev["pdf"]))
    # against float64, within twice part 1's measured error (F at the same rounded wavelength)
    inside = (mr.index32(lam) >= 0) & (mr.index32(lam) < mr.NSPEC) & (wi[:, 0] == wi[:, 0])
    n64, k64 = (a[np.clip(mr.index32(lam), 0, 470)] for a in mr.nk64(mr.METALS[metal]))
    ss, tt = rr.frame32(nrm)
    ch = mr.cos_h32(rr.to_local32(-d, ss, tt, nrm), rr.to_local32(wi, ss, tt, nrm)).astype(np.float64)
    assert np.max(np.abs(got["F"][inside] - mr.F64(ch, n64, k64)[inside])) <= mr.bounds()["F"]


def test_debug_entries_are_guarded(floor):
    F = C.POINTER(C.c_float)
    v = np.array([[0.0, 0.0, 1.0]], f32)
    o = np.full(4, 550.0, f32)
    p = lambda a: a.ctypes.data_as(F)
    lib, h = floor.lib, floor.h
    ok = lambda *a: lib.rt_debug_conductor_eval(h, *a)
    assert ok(2, 0.5, 1, p(v), p(v), p(v), p(o), p(o), p(o), p(o)) == capi.RT_OK
    for alpha in (0.0, 0.009, 1.01, float("nan"), -1.0):
        assert ok(2, alpha, 1, p(v), p(v), p(v), p(o), p(o), p(o), p(o)) == capi.RT_E_ARG
    for metal in (-1, 4):
        assert ok(metal, 0.5, 1, p(v), p(v), p(v), p(o), p(o), p(o), p(o)) == capi.RT_E_ARG
    assert ok(2, 0.5, -1, p(v), p(v), p(v), p(o), p(o), p(o), p(o)) == capi.RT_E_ARG
    for k in range(7):
        a = [p(v), p(v), p(v), p(o), p(o), p(o), p(o)]
        a[k] = None
        assert ok(2, 0.5, 1, *a) == capi.RT_E_ARG, k
    assert lib.rt_debug_conductor_stats(h, None) == capi.RT_E_ARG


# ------------------------------------------------------------------------------------------ 2. validation

def _metal_floor_cfg(alpha=0.5, sig=(2.0, 0.0, 0.0), emit=0.0):
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(ref.K2_DIR), scale=0.1)])
    m.materials[0] = (tuple(sig), emit, capi.RT_MAT_CONDUCTOR, alpha)
    return ref._config("metal_validation", m, ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1, film=ref._film())


def test_upload_validates_a_conductor_and_keeps_the_scene():
    g = Renderer(_metal_floor_cfg())
    try:
        before = g.render_pass(0, 4)
        assert g.conductor_launches() > 0 and before[:, :3].max() > 0
        nan = float("nan")
        bad = [dict(alpha=a) for a in (0.0, 0.009, 1.01, nan)]
        bad += [dict(sig=(m, 0.0, 0.0)) for m in (-1.0, 4.0, 0.5, nan)]
        bad += [dict(sig=(2.0, 1e-3, 0.0)), dict(sig=(2.0, 0.0, -2.0))]
        for kw in bad:
            d = _metal_floor_cfg(**kw).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG, kw
            if "alpha" in kw:
                assert b"alpha" in g.lib.rt_last_error(g.h)
            # the scene bound before stays
            assert np.array_equal(bits(g.render_pass(0, 4)), bits(before)), kw
        for kw in (dict(alpha=0.01), dict(alpha=1.0), dict(sig=(0.0, 0.0, 0.0)), dict(sig=(3.0, 0.0, 0.0))):
            d = _metal_floor_cfg(**kw).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_OK, kw
        d = ref._floor_model(False).desc()
        d.materials[0].type = 5
        assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG
    finally:
        g.close()


def test_emissive_type_4_is_an_emitter():
    """An emitter of type 4 shades as an emitter of type 0 does (its type, eta and sigmoid are never read), bit for bit, and
    launches no level-2 instantiation."""
    films = []
    for typ in (capi.RT_MAT_DIFFUSE, capi.RT_MAT_CONDUCTOR):
        cfg = ref.k3_quad(mis=True, max_depth=2, seen=True)[0]
        mats = list(cfg.model.materials)
        mats[1] = (mats[1][0], mats[1][1], typ, 0.0)
        cfg.model.materials = mats
        g = Renderer(cfg)
        try:
            films.append(g.render_pass(0, 16))
            assert g.conductor_launches() == 0 and g.rough_launches() == 0
        finally:
            g.close()
    assert films[0][:, :3].max() > 0 and np.array_equal(bits(films[0]), bits(films[1]))


def test_no_texture_binds_to_a_conductor():
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(ref.K2_DIR), scale=0.1)])
    m.texcoords = np.full((len(m.positions), 2), 0.5, f32)
    m.textures = [scene.Texture(np.full((1, 1, 3), 128, np.uint8), wrap="clamp")]
    m.material_texture = [0] + [-1] * (len(m.materials) - 1)
    cfg = ref._config("metal_texture", m, ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1, film=ref._film())
    g = Renderer(cfg)                                          # (a texture on the Lambert floor binds)
    try:
        m.materials[0] = scene.metal("Au", 0.5)
        with pytest.raises(capi.RTError) as e:
            g.configure(cfg)                                   # (the upload succeeds, the binding is refused)
        assert e.value.status == capi.RT_E_ARG and "conductor" in str(e.value)
        # the gold floor renders untextured
        film = g.render_pass(0, 4)
        assert g.conductor_launches() > 0 and film[:, :3].max() > 0
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 3. instantiations

def _with(cfg, which, mat):
    mats = [tuple(m) for m in cfg.model.materials]
    mats[which] = mat(mats[which]) if callable(mat) else mat
    cfg.model.materials = mats
    return cfg


@pytest.mark.parametrize("name", ["cornell", "cfg4"])
def test_level_2_instantiations_run_only_with_a_conductor(name):
    make = {"cornell": lambda: scene.cfg_cornell(res=(32, 32), spp_side=2),
            "cfg4": lambda: scene.cfg4_mixed(res=(48, 27), spp=(2, 2), frequency=8)}[name]
    g = Renderer(make())
    try:
        plain = g.render_pass(0, 4)
        assert g.conductor_launches() == 0 and g.rough_launches() == 0, "as shipped"
        g.configure(_with(make(), 0, lambda m: scene.rough(m[0], 0.3)))
        rough = g.render_pass(0, 4)
        n_rough = g.rough_launches()
        assert g.conductor_launches() == 0 and n_rough > 0, "a rough-only scene runs level 1"
        g.configure(_with(make(), 0, scene.metal("Au", 0.3)))
        gold = g.render_pass(0, 4)
        assert g.conductor_launches() > 0 and g.conductor_launches() == g.rough_launches() == n_rough
        assert np.all(np.isfinite(gold)) and not np.array_equal(bits(gold), bits(rough))
        assert g.stats()["coop_overflows"] == 0
        g.configure(_with(make(), 0, lambda m: scene.rough(m[0], 0.3)))
        assert np.array_equal(bits(g.render_pass(0, 4)), bits(rough)) and g.conductor_launches() == 0
        assert g.rough_launches() == n_rough
        g.configure(make())
        again = g.render_pass(0, 4)
        assert g.conductor_launches() == 0 and g.rough_launches() == 0, "after re-uploading without one"
        assert np.array_equal(bits(again), bits(plain)), "the scene without a conductor renders what it rendered"
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 4. films against float64

def _render(cfg, env=None, spans=((0, SPP),)):
    g = Renderer(cfg)
    try:
        if env is not None:
            g.set_environment(env)
        oc = g.octree()
        depth = oc["depth"], oc["max_queue_groups"]
        film = None
        for a, b in spans:
            film = g.render_pass(a, b, film)
        return film, depth, g.conductor_launches()
    finally:
        g.close()


def _check(name, film, mu, vmax, include):
    rows = ref.compare(film, mu, vmax, include, SPP)
    print(f"\n{name}: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), name
    for k in (1.03, 0.97):
        assert not ref.passes(ref.compare(film, mu * k, vmax, include, SPP)), f"{name}: mu x {k} passes too"


def _closed_form(name, case, multi_level=None):
    """The film against mu on the whole frame and each quadrant, by radiometry_reference.tolerance; the same film must
    fail against mu x 1.03 and mu x 0.97."""
    env = case[1] if isinstance(case[1], scene.Environment) else None
    cfg, (mu, vmax, include) = case[0], (case[2:5] if env is not None else case[1:4])
    assert np.all(vmax < 1.0)
    film, depth, launches = _render(cfg, env)
    if multi_level is not None:
        assert (depth[0] > 0) == multi_level, depth
        assert (depth[1] > 16) == multi_level, depth   # (QCAP 0 with coop_ok: DESIGN §2)
    assert launches > 0
    _check(name, film, mu, vmax, include)
    return film


@pytest.mark.parametrize("alpha,tessellated", [(0.5, False), (0.5, True), (0.2, False), (0.2, True)])
def test_m1_distant_light_on_the_gold_floor(alpha, tessellated):
    case = mr.m1_distant("Au", alpha, tessellated)
    mu = case[1]
    # a grey floor has Z / X = 1.089 / 0.950 = 1.15 under D65; gold's F(1) is 0.39 at 450 nm and 0.94 at 650 nm
    assert mu[:, 2].mean() < 0.7 * mu[:, 0].mean(), "gold: the XYZ channels differ"
    _closed_form(f"M1 alpha {alpha} {'multi-level' if tessellated else 'single-leaf'}", case, multi_level=tessellated)


def test_m1g_gold_floor_at_grazing_angles():
    """wo.h <= 0.35 on every pixel (about 0.11): tests/test_metal_reference.py checks on the CPU that F(lambda, 1) at every
    angle and Schlick from F(1) each move this case's Z mean by more than twice its tolerance."""
    _closed_form("M1g", mr.m1_distant("Au", 0.5, graze=True))


@pytest.mark.parametrize("mis", [False, True])
def test_m2_quad_light_on_the_copper_floor(mis):
    _closed_form(f"M2 {'PATH_MIS' if mis else 'PATH'}", mr.m2_quad("Cu", 0.3, mis))


@pytest.mark.parametrize("mis,depth", [(False, 1), (True, 1), (True, 5)])
def test_m3_gold_sphere_under_a_constant_map(mis, depth):
    _closed_form(f"M3 {'PATH_MIS' if mis else 'PATH'} depth {depth}", mr.m3_sphere("Au", mis, depth))


def test_m4_gold_floor_seen_in_a_mirror_wall():
    """Incoming beta != 1 ahead of a conductor vertex, the class-0 and class-1 bins in one pass: the whole frame, and the
    pixels that show the floor's mirror image on their own."""
    cfg, mu, vmax, include, seen_mirror = mr.m1_distant("Au", 0.5, True, mirror=True)
    film = _closed_form("M4", (cfg, mu, vmax, include), multi_level=True)
    _check("M4 mirror image alone", film, mu, vmax, seen_mirror)
    # without the mirror's R = 0.9 the mirror image alone would be 11 % too bright
    assert not ref.passes(ref.compare(film, mu / mr.M4_R, vmax, seen_mirror, SPP))


def test_m5_rough_and_conductor_halves_in_one_launch():
    cfg, mu, vmax, include, rough_half = mr.m1_distant("Au", 0.5, True, half_rough=True)
    film = _closed_form("M5", (cfg, mu, vmax, include), multi_level=True)
    _check("M5 rough half", film, mu, vmax, include & rough_half)
    _check("M5 gold half", film, mu, vmax, include & ~rough_half)


def test_m6_aluminium_floor_on_the_sony_sensor():
    _closed_form("M6", mr.m1_distant("Al", 0.5, sensor="sony_ilce_6400"))


# ------------------------------------------------------------------------------------------ 5. split passes

@pytest.mark.parametrize("which", ["m1", "m1_multi", "m3"])
def test_split_passes_give_one_pass_bits(which):
    case = {"m1": lambda: mr.m1_distant("Au", 0.5), "m1_multi": lambda: mr.m1_distant("Au", 0.2, True),
            "m3": lambda: mr.m3_sphere("Au", True, 5)}[which]()
    env = case[1] if isinstance(case[1], scene.Environment) else None
    one = _render(case[0], env)[0]
    two = _render(case[0], env, spans=((0, 128), (128, 256)))[0]
    assert np.array_equal(bits(one), bits(two))


def test_albedo_film_leaves_a_conductor_undemodulated():
    """rt_render_features_albedo: every camera ray hits the gold floor, so each pixel holds k (1, 1, 1, 1)."""
    g = Renderer(mr.m1_distant("Au", 0.5)[0])
    try:
        _, _, alb = g.render_features_albedo(0, 3)
    finally:
        g.close()
    assert np.array_equal(bits(alb), bits(np.full(alb.shape, 3.0, f32)))
