"""The rough reflector (RT_MAT_ROUGH) on the device: the shade kernel's GGX device functions bit for bit
against tests/rough_reference.py, rt_scene_upload's validation, which instantiations a scene runs, films against float64
closed forms, split passes and the albedo film.  The oracle does not know this material: nothing here renders through it.

Film cases built here: G1 (distant light, alpha 0.5 and 0.2, single-leaf and multi-level), G2 (quad light, PATH and
PATH_MIS), G3 (sphere under a constant map: PATH depth 1, PATH_MIS depth 1 and 5), G3m (the sphere in an emissive box
declared as a mesh light), G4 (the floor seen in a mirror wall), G5 (red floor, Sony sensor), G6 (a one-texel texture).  The measured |got - mu| / tol of each is recorded in DESIGN.md §3k.
"""
import ctypes as C

import numpy as np
import pytest

import albedo_reference as aref
import camera_reference
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
    """One context over the plain Lambert floor: the debug entries and the validation tests use it."""
    cfg = ref._config("rough_floor", ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,
                      film=ref._film())
    g = Renderer(cfg)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------ 1. the device functions

def _debug_inputs(n=4096, seed=5):
    """Unit normals all over the sphere (both branches of the frame's sign(nrm.z), the poles among them), incoming
    directions against the normal from grazing to head-on, sample points with the centre, the rim and the corners."""
    rng = np.random.default_rng(seed)
    nrm = rr.nrm64(rng.normal(size=(n, 3)))
    nrm[:4] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]]
    assert (nrm[:, 2] < 0).sum() > n // 3
    t = rr.nrm64(np.cross(nrm, rng.normal(size=(n, 3))))
    mu = np.concatenate([np.full(64, 1e-3), np.geomspace(1e-3, 1.0, 512), rng.random(n - 64 - 512 - 64), np.full(64, 1.0)])
    d = -(mu[:, None] * nrm + np.sqrt(1 - mu * mu)[:, None] * t)
    u = rng.random((n, 2))
    u[:8] = [[0.5, 0.5], [0, 0], [1, 1], [0, 1], [1, 0.5], [0.5, 0], [0, 0.5], [0.5, 1]]
    wi = rr.nrm64(rng.normal(size=(n, 3)))
    flip = np.sum(wi * nrm, -1) < 0
    wi[flip & (np.arange(n) % 8 != 0)] *= -1                 # (an eighth of those below the horizon stay there)
    as32 = lambda a: rr.norm32(a.astype(f32))
    u32 = np.clip(u.astype(f32), f32(0), np.nextafter(f32(1), f32(0)))         # (samplers draw from [0, 1))
    return as32(nrm), as32(d), u32, as32(wi)


@pytest.mark.parametrize("alpha", [0.01, 0.2, 1.0])
def test_device_functions_bit_for_bit(floor, alpha):
    nrm, d, u, wi = _debug_inputs()
    got = floor.ggx_sample(alpha, nrm, d, u)
    # the disk point: the project's disk_concentric against the float64 map, within 4 ulp of 1
    want_disk = camera_reference.concentric_disk(u.astype(np.float64))
    assert np.max(np.abs(got["disk"].astype(np.float64) - want_disk)) <= 4 * 2.0 ** -23
    # everything after it from the device's own disk point: no item is excluded
    w, wb, pdf, ok = rr.debug_sample32(alpha, nrm, d, got["disk"])
    assert 0.3 < ok.mean() < 1.0
    assert np.array_equal(bits(got["wi"]), bits(w)), f"{np.sum(np.any(bits(got['wi']) != bits(w), axis=1))} wi differ"
    assert np.array_equal(bits(got["wb"]), bits(wb)), f"{np.sum(bits(got['wb']) != bits(wb))} wb differ"
    assert np.array_equal(bits(got["pdf"]), bits(pdf)), f"{np.sum(bits(got['pdf']) != bits(pdf))} pdfs differ"
    ev = floor.ggx_eval(alpha, nrm, d, wi)
    fc, pe = rr.debug_eval32(alpha, nrm, d, wi)
    assert (fc == 0).sum() > 100 and (fc > 0).sum() > 2000
    assert np.array_equal(bits(ev["fcos"]), bits(fc)), f"{np.sum(bits(ev['fcos']) != bits(fc))} fcos differ"
    assert np.array_equal(bits(ev["pdf"]), bits(pe)), f"{np.sum(bits(ev['pdf']) != bits(pe))} pdfs differ"
    # the sampled direction evaluates to the sampled pdf up to the half vector's float32 round trip
    back = floor.ggx_eval(alpha, nrm, d, got["wi"])
    sel = ok & (rr.to_local32(got["wi"], *rr.frame32(nrm), nrm)[:, 2] > 1e-2)
    if alpha >= 0.2:
        assert np.allclose(back["pdf"][sel], got["pdf"][sel], rtol=1e-3)


def test_debug_entries_are_guarded(floor):
    F = C.POINTER(C.c_float)
    v = np.array([[0.0, 0.0, 1.0]], f32)
    o = np.zeros(4, f32)
    p = lambda a: a.ctypes.data_as(F)
    lib, h = floor.lib, floor.h
    assert lib.rt_debug_ggx_eval(h, 0.5, 1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_OK
    for alpha in (0.0, 0.009, 1.01, float("nan"), -1.0):
        assert lib.rt_debug_ggx_eval(h, alpha, 1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
        assert lib.rt_debug_ggx_sample(h, alpha, 1, p(v), p(v), p(o), p(o), p(o), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_ggx_eval(h, 0.5, -1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_ggx_eval(h, 0.5, 1, None, p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_ggx_sample(h, 0.5, 1, p(v), p(v), p(o), None, p(o), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_rough_stats(h, None) == capi.RT_E_ARG


# ------------------------------------------------------------------------------------------ 2. validation

def _rough_floor_cfg(alpha, emit=0.0):
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(ref.K2_DIR), scale=0.1)])
    m.materials[0] = (scene.grey_sigmoid(0.5), emit, capi.RT_MAT_ROUGH, alpha)
    return ref._config("rough_validation", m, ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1, film=ref._film())


def test_upload_validates_alpha_and_keeps_the_scene():
    g = Renderer(_rough_floor_cfg(0.5))
    try:
        before = g.render_pass(0, 4)
        assert g.rough_launches() > 0
        for alpha in (0.0, 0.009, 1.01, float("nan"), -0.3):
            d = _rough_floor_cfg(alpha).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG, alpha
            assert b"alpha" in g.lib.rt_last_error(g.h)
            # the scene bound before stays
            assert np.array_equal(bits(g.render_pass(0, 4)), bits(before)), alpha
        for alpha in (0.01, 1.0):
            d = _rough_floor_cfg(alpha).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_OK, alpha
        d = ref._floor_model(False).desc()
        d.materials[0].type = 4
        assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG
    finally:
        g.close()


def test_emissive_type_3_is_an_emitter():
    """An emitter of type 3 shades as an emitter of type 0 does (the type of an emitter is never read), bit for bit, and
    launches no RGH instantiation."""
    films = []
    for typ in (capi.RT_MAT_DIFFUSE, capi.RT_MAT_ROUGH):
        cfg = ref.k3_quad(mis=True, max_depth=2, seen=True)[0]
        mats = list(cfg.model.materials)
        mats[1] = (mats[1][0], mats[1][1], typ, 0.0)
        cfg.model.materials = mats
        g = Renderer(cfg)
        try:
            films.append(g.render_pass(0, 16))
            assert g.rough_launches() == 0
        finally:
            g.close()
    assert films[0][:, :3].max() > 0 and np.array_equal(bits(films[0]), bits(films[1]))


# ------------------------------------------------------------------------------------------ 3. instantiations

def _with_rough(cfg, which, alpha=0.3):
    mats = [tuple(m) for m in cfg.model.materials]
    mats[which] = scene.rough(mats[which][0], alpha)
    cfg.model.materials = mats
    return cfg


@pytest.mark.parametrize("name", ["cornell", "cfg4"])
def test_rgh_instantiations_run_only_with_a_rough_material(name):
    make = {"cornell": lambda: scene.cfg_cornell(res=(32, 32), spp_side=2),
            "cfg4": lambda: scene.cfg4_mixed(res=(48, 27), spp=(2, 2), frequency=8)}[name]
    cfg = make()
    g = Renderer(cfg)
    try:
        plain = g.render_pass(0, 4)
        assert g.rough_launches() == 0, "as shipped"
        g.configure(_with_rough(make(), 0))
        rough = g.render_pass(0, 4)
        assert g.rough_launches() > 0
        assert np.all(np.isfinite(rough)) and not np.array_equal(bits(rough), bits(plain))
        assert g.stats()["coop_overflows"] == 0
        g.configure(make())
        again = g.render_pass(0, 4)
        assert g.rough_launches() == 0, "after re-uploading without one"
        assert np.array_equal(bits(again), bits(plain)), "the scene without a rough material renders what it rendered"
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
        return film, depth, g.rough_launches()
    finally:
        g.close()


def _closed_form(name, case, multi_level=None):
    """The film against mu on the whole frame and each quadrant, by radiometry_reference.tolerance; the same film must
    fail against mu x 1.03 and mu x 0.97."""
    cfg, mu, vmax, include = case[0], case[-3], case[-2], case[-1]
    env = case[1] if len(case) == 5 else None
    assert np.all(vmax < 1.0)
    film, depth, launches = _render(cfg, env)
    if multi_level is not None:
        assert (depth[0] > 0) == multi_level, depth
        assert (depth[1] > 16) == multi_level, depth   # (QCAP 0 with coop_ok: DESIGN §2)
    assert launches > 0
    rows = ref.compare(film, mu, vmax, include, SPP)
    print(f"\n{name}: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), name
    for k in (1.03, 0.97):
        assert not ref.passes(ref.compare(film, mu * k, vmax, include, SPP)), f"{name}: mu x {k} passes too"
    return film


@pytest.mark.parametrize("alpha,tessellated", [(0.5, False), (0.5, True), (0.2, False), (0.2, True)])
def test_g1_distant_light_on_the_rough_floor(alpha, tessellated):
    _closed_form(f"G1 alpha {alpha} {'multi-level' if tessellated else 'single-leaf'}",
                 rr.g1_distant(alpha, tessellated), multi_level=tessellated)


@pytest.mark.parametrize("mis", [False, True])
def test_g2_quad_light_on_the_rough_floor(mis):
    _closed_form(f"G2 {'PATH_MIS' if mis else 'PATH'}", rr.g2_quad(0.3, mis))


@pytest.mark.parametrize("mis,depth", [(False, 1), (True, 1), (True, 5)])
def test_g3_rough_sphere_under_a_constant_map(mis, depth):
    _closed_form(f"G3 {'PATH_MIS' if mis else 'PATH'} depth {depth}", rr.g3_sphere(mis, depth))


@pytest.mark.parametrize("depth", [1, 5])
def test_g3m_rough_sphere_in_the_emissive_box(depth):
    """G3 through mesh-light NEE and the BSDF-sampled emitter hit."""
    _closed_form(f"G3m depth {depth}", rr.g3m_box(depth))


def test_g4_rough_floor_seen_in_a_mirror_wall():
    """Incoming beta != 1 and prevPdf = 0 ahead of a rough vertex, the class-0 and class-1 bins in one pass: the whole
    frame, and the pixels that show the floor's mirror image on their own."""
    cfg, mu, vmax, include, seen_mirror = rr.g4_mirror()
    film = _closed_form("G4", (cfg, mu, vmax, include), multi_level=True)
    rows = ref.compare(film, mu, vmax, seen_mirror, SPP)
    print(f"G4 mirror image alone: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows)
    for k in (1.03, 0.97):
        assert not ref.passes(ref.compare(film, mu * k, vmax, seen_mirror, SPP))
    # without the mirror's R = 0.9 the mirror image alone would be 11 % too bright
    assert not ref.passes(ref.compare(film, mu / rr.G4_R, vmax, seen_mirror, SPP))


def test_g5_red_floor_on_the_sony_sensor():
    case = rr.g1_distant(0.5, albedo_c=ref.S_RED, sensor="sony_ilce_6400")
    mu = case[1]
    assert mu[:, 2].mean() < 0.25 * mu[:, 0].mean(), "response(R), not grey"
    _closed_form("G5", case)


def test_g6_one_texel_texture_on_the_rough_floor():
    """TEX x RGH: the texel supplies R; the film has the untextured closed form at R = 128 / 255 (the material's own
    sigmoid, 0.25, would be far outside the tolerance)."""
    _closed_form("G6", rr.g1_distant(0.5, texture=True))


# ------------------------------------------------------------------------------------------ 5. split passes, albedo

@pytest.mark.parametrize("which", ["g1", "g1_multi", "g3"])
def test_split_passes_give_one_pass_bits(which):
    case = {"g1": lambda: rr.g1_distant(0.5), "g1_multi": lambda: rr.g1_distant(0.2, True),
            "g3": lambda: rr.g3_sphere(True, 5)}[which]()
    env = case[1] if len(case) == 5 else None
    one = _render(case[0], env)[0]
    two = _render(case[0], env, spans=((0, 128), (128, 256)))[0]
    assert np.array_equal(bits(one), bits(two))


def test_albedo_film_of_a_rough_floor():
    """rt_render_features_albedo demodulates a rough surface by A of its material, like Lambert: every camera ray hits
    the floor, so each pixel holds k (A, 1) summed in index order."""
    cfg = rr.g1_distant(0.5, albedo_c=ref.S_RED)[0]
    g = Renderer(cfg)
    try:
        _, _, alb = g.render_features_albedo(0, 3)
    finally:
        g.close()
    bars, d65 = aref.dense_tables("xyz")
    A = aref.sensor_albedo(np.array(cfg.model.materials[0][0], f32), bars, d65)
    assert np.all(A > 0) and np.all(A < 1) and A[0] > 2 * A[2]
    one = np.concatenate([A, [f32(1)]]).astype(f32)
    want = (one + one) + one
    assert np.array_equal(bits(alb), bits(np.broadcast_to(want, alb.shape)))
