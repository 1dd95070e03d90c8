"""Rough glass (RT_MAT_ROUGH_DIELECTRIC) on the device: the level-3 kernels' device functions bit for bit
against tests/roughglass_reference.py, rt_scene_upload's validation, which instantiations a scene runs, films against
float64 closed forms, split passes and the albedo film.  The oracle does not know this material: nothing here renders
through it.

Film cases built here: D1 (distant light, alpha 0.5 and 0.2, single-leaf and multi-level), D2 (quad light, PATH and
PATH_MIS), D3 (the floor alone under a constant map from above: PATH depth 1, PATH_MIS depth 1 and 5), D3b (from below:
back faces, er = 1 / eta, pixels past the critical angle), D4 (a quad emitter below the floor, PATH and PATH_MIS), D5
(gold, rough glass and rough grey in one level-3 pass), D6 (D3 with a mirror wall, depth 2, PATH and PATH_MIS) and D6d
(the wall under D1's distant light).  The
measured |got - mu| / tol of each is recorded in DESIGN.md §3m.
"""
import ctypes as C

import numpy as np
import pytest

import camera_reference
import radiometry_reference as ref
import rough_reference as rr
import roughglass_reference as rg
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
f32 = np.float32
SPP = 256
ONE_M = np.nextafter(f32(1), f32(0))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def floor():
    """One context over the plain Lambert floor: the debug entries use it."""
    cfg = ref._config("roughglass_floor", ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,
                      film=ref._film())
    g = Renderer(cfg)
    yield g
    g.close()


# ------------------------------------------------------------------------------------------ 1. the device functions

def _debug_inputs(n=4096, seed=5):
    """test_gpu_rough's inputs (unit normals all over the sphere, incoming directions from grazing to head-on, sample
    points with the centre, the rim and the corners) and the Fresnel choice's u with 0 and nextafter(1, 0)."""
    rng = np.random.default_rng(seed)
    nrm = rr.nrm64(rng.normal(size=(n, 3)))
    nrm[:4] = [[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0]]
    t = rr.nrm64(np.cross(nrm, rng.normal(size=(n, 3))))
    mu = np.concatenate([np.full(64, 1e-3), np.geomspace(1e-3, 1.0, 512), rng.random(n - 64 - 512 - 64), np.full(64, 1.0)])
    d = -(mu[:, None] * nrm + np.sqrt(1 - mu * mu)[:, None] * t)
    u = rng.random((n, 3))
    u[:8, :2] = [[0.5, 0.5], [0, 0], [1, 1], [0, 1], [1, 0.5], [0.5, 0], [0, 0.5], [0.5, 1]]
    u[8::61, 2] = 0.0
    u[9::61, 2] = 1.0
    wi = rr.nrm64(rng.normal(size=(n, 3)))
    flip = np.sum(wi * nrm, -1) < 0
    wi[flip & (np.arange(n) % 8 != 0)] *= -1                 # (an eighth of those below the horizon stay there)
    as32 = lambda a: rr.norm32(a.astype(f32))
    u32 = np.clip(u.astype(f32), f32(0), ONE_M)              # (samplers draw from [0, 1))
    return as32(nrm), as32(d), u32, as32(wi)


@pytest.mark.parametrize("er", [1.5, 1 / 1.5])
@pytest.mark.parametrize("alpha", [0.01, 0.2, 1.0])
def test_device_functions_bit_for_bit(floor, alpha, er):
    nrm, d, u, wi = _debug_inputs()
    got = floor.roughglass_sample(alpha, er, nrm, d, u)
    want_disk = camera_reference.concentric_disk(u[:, :2].astype(np.float64))
    assert np.max(np.abs(got["disk"].astype(np.float64) - want_disk)) <= 4 * 2.0 ** -23
    # everything after the disk point from the device's own: no item is excluded
    w, wt, pdf, br = rg.debug_sample32(alpha, er, nrm, d, got["disk"], u[:, 2])
    assert np.all(np.bincount(br, minlength=3)[1:] > 100) and (br == 0).any(), np.bincount(br, minlength=3)
    assert np.array_equal(got["branch"], br), f"{np.sum(got['branch'] != br)} branches differ"
    assert np.array_equal(bits(got["wi"]), bits(w)), f"{np.sum(np.any(bits(got['wi']) != bits(w), axis=1))} wi differ"
    assert np.array_equal(bits(got["w"]), bits(wt)), f"{np.sum(bits(got['w']) != bits(wt))} weights differ"
    assert np.array_equal(bits(got["pdf"]), bits(pdf)), f"{np.sum(bits(got['pdf']) != bits(pdf))} pdfs differ"
    ev = floor.roughglass_eval(alpha, er, nrm, d, wi)
    fc, pe = rg.debug_eval32(alpha, er, nrm, d, wi)
    assert (fc == 0).sum() > 100 and (fc > 0).sum() > 2000
    assert np.array_equal(bits(ev["fcos"]), bits(fc)), f"{np.sum(bits(ev['fcos']) != bits(fc))} fcos differ"
    assert np.array_equal(bits(ev["pdf"]), bits(pe)), f"{np.sum(bits(ev['pdf']) != bits(pe))} pdfs differ"
    # the host functions give the device's bits on the device's local vectors
    ss, tt = rr.frame32(nrm)
    wol = rr.to_local32(-d, ss, tt, nrm)
    hw, hwt, hp, hb = scene.roughglass_sample(alpha, er, wol, got["disk"], u[:, 2])
    assert np.array_equal(hb, got["branch"]) and np.array_equal(bits(hwt), bits(got["w"]))
    assert np.array_equal(bits(hp), bits(got["pdf"]))


def test_debug_entries_are_guarded(floor):
    F = C.POINTER(C.c_float)
    v = np.array([[0.0, 0.0, 1.0]], f32)
    o = np.zeros(4, f32)
    b = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(F)
    pb = b.ctypes.data_as(C.POINTER(C.c_int32))
    lib, h = floor.lib, floor.h
    assert lib.rt_debug_roughglass_eval(h, 0.5, 1.5, 1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_OK
    for alpha in (0.0, 0.009, 1.01, float("nan"), -1.0):
        assert lib.rt_debug_roughglass_eval(h, alpha, 1.5, 1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
        assert lib.rt_debug_roughglass_sample(h, alpha, 1.5, 1, p(v), p(v), p(v), p(o), p(o), p(o), p(o), pb) == capi.RT_E_ARG
    for er in (0.0, -1.5, float("nan"), float("inf")):
        assert lib.rt_debug_roughglass_eval(h, 0.5, er, 1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_roughglass_eval(h, 0.5, 1.5, -1, p(v), p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_roughglass_eval(h, 0.5, 1.5, 1, None, p(v), p(v), p(o), p(o)) == capi.RT_E_ARG
    assert lib.rt_debug_roughglass_sample(h, 0.5, 1.5, 1, p(v), p(v), p(v), p(o), None, p(o), p(o), pb) == capi.RT_E_ARG
    assert lib.rt_debug_roughglass_stats(h, None) == capi.RT_E_ARG


# ------------------------------------------------------------------------------------------ 2. validation

def _glass_floor_cfg(eta=1.5, alpha=0.5, c1=0.0, c2=0.0, emit=0.0):
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(ref.K2_DIR), scale=0.1)])
    m.materials[0] = ((alpha, c1, c2), emit, capi.RT_MAT_ROUGH_DIELECTRIC, eta)
    return ref._config("roughglass_validation", m, ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1, film=ref._film())


def test_upload_validates_and_keeps_the_scene():
    g = Renderer(_glass_floor_cfg())
    try:
        before = g.render_pass(0, 4)
        assert g.roughglass_launches() > 0 and before[:, :3].max() > 0
        bad = [dict(alpha=a) for a in (0.0, 0.009, 1.01, float("nan"))]
        bad += [dict(eta=e) for e in (0.0, 1.0, 0.9, float("nan"), float("inf"))]
        bad += [dict(c1=0.5), dict(c2=-1.0)]
        for kw in bad:
            d = _glass_floor_cfg(**kw).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG, kw
            msg = g.lib.rt_last_error(g.h)
            if "alpha" in kw:
                assert b"alpha" in msg
            if kw.get("eta") == 0.0:
                assert b"dispersive" in msg
            # the scene bound before stays
            assert np.array_equal(bits(g.render_pass(0, 4)), bits(before)), kw
        for kw in (dict(alpha=0.01), dict(alpha=1.0), dict(eta=1.0001), dict(eta=2.4)):
            d = _glass_floor_cfg(**kw).model.desc()
            assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_OK, kw
        d = ref._floor_model(False).desc()
        d.materials[0].type = 6
        assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_E_ARG
    finally:
        g.close()


def test_emissive_type_5_is_an_emitter():
    """An emitter of type 5 shades as an emitter of type 0 does (an emitter's fields are never validated or read), bit
    for bit, and launches no level-3 instantiation."""
    films = []
    for typ, eta, sig in ((capi.RT_MAT_DIFFUSE, 0.0, (0.0, 0.0, 0.0)), (capi.RT_MAT_ROUGH_DIELECTRIC, 0.0, (7.0, 1.0, 1.0))):
        cfg = ref.k3_quad(mis=True, max_depth=2, seen=True)[0]
        mats = list(cfg.model.materials)
        mats[1] = (sig, mats[1][1], typ, eta)
        cfg.model.materials = mats
        g = Renderer(cfg)
        try:
            films.append(g.render_pass(0, 16))
            assert g.roughglass_launches() == 0
        finally:
            g.close()
    assert films[0][:, :3].max() > 0 and np.array_equal(bits(films[0]), bits(films[1]))


def test_a_texture_on_rough_glass_is_refused():
    m = ref._floor_model(False, lights=[dict(type=capi.RT_LIGHT_DISTANT, dir=tuple(ref.K2_DIR), scale=0.1)])
    m.texcoords = np.full((len(m.positions), 2), 0.5, f32)
    m.textures = [scene.Texture(np.full((1, 1, 3), 128, np.uint8), wrap="clamp")]
    m.material_texture = [0] + [-1] * (len(m.materials) - 1)
    cfg = ref._config("roughglass_texture", m, ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1, film=ref._film())
    g = Renderer(cfg)                                          # (a texture on the Lambert floor binds)
    try:
        m.materials[0] = scene.rough_glass(1.5, 0.5)
        with pytest.raises(capi.RTError) as e:
            g.configure(cfg)                                   # (the upload succeeds, the binding is refused)
        assert e.value.status == capi.RT_E_ARG and "rough dielectric" in str(e.value)
        film = g.render_pass(0, 4)                             # the glass floor renders untextured
        assert g.roughglass_launches() > 0 and film[:, :3].max() > 0
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 3. instantiations

def _with(cfg, which, mat):
    mats = [tuple(m) for m in cfg.model.materials]
    mats[which] = mat(mats[which])
    cfg.model.materials = mats
    return cfg


_GLASS = lambda m: scene.rough_glass(1.5, 0.3)
_ROUGH = lambda m: scene.rough(m[0], 0.3)
_GOLD = lambda m: scene.metal("Au", 0.3)


@pytest.mark.parametrize("name", ["cornell", "cfg4", "rough_only", "conductor_only"])
def test_level_3_runs_only_with_a_rough_glass(name):
    base = {"cornell": lambda: scene.cfg_cornell(res=(32, 32), spp_side=2),
            "cfg4": lambda: scene.cfg4_mixed(res=(48, 27), spp=(2, 2), frequency=8),
            "rough_only": lambda: _with(scene.cfg_cornell(res=(32, 32), spp_side=2), 0, _ROUGH),
            "conductor_only": lambda: _with(scene.cfg4_mixed(res=(48, 27), spp=(2, 2), frequency=8), 0, _GOLD)}[name]
    g = Renderer(base())
    try:
        plain = g.render_pass(0, 4)
        counters = (g.rough_launches(), g.conductor_launches())
        assert g.roughglass_launches() == 0, "as shipped"
        assert (counters[0] > 0) == (name in ("rough_only", "conductor_only")) and (counters[1] > 0) == (name == "conductor_only")
        g.configure(_with(base(), 1, _GLASS))
        glass = g.render_pass(0, 4)
        assert g.roughglass_launches() > 0
        # level 3 is an RGH level: the rough counter ticks with it; the conductor counter only with a conductor in the scene
        assert g.rough_launches() == g.roughglass_launches()
        assert g.conductor_launches() == (g.roughglass_launches() if name == "conductor_only" else 0)
        assert np.all(np.isfinite(glass)) and not np.array_equal(bits(glass), bits(plain))
        assert g.stats()["coop_overflows"] == 0
        g.configure(base())
        again = g.render_pass(0, 4)
        assert g.roughglass_launches() == 0, "after re-uploading without one"
        assert (g.rough_launches(), g.conductor_launches()) == counters
        assert np.array_equal(bits(again), bits(plain)), "the scene without a rough glass renders what it rendered"
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
        return film, depth, g.roughglass_launches()
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
def test_d1_distant_light_on_the_rough_glass_floor(alpha, tessellated):
    _closed_form(f"D1 alpha {alpha} {'multi-level' if tessellated else 'single-leaf'}",
                 rg.d1_distant(alpha, tessellated), multi_level=tessellated)


@pytest.mark.parametrize("mis", [False, True])
def test_d2_quad_light_on_the_rough_glass_floor(mis):
    _closed_form(f"D2 {'PATH_MIS' if mis else 'PATH'}", rg.d2_quad(0.3, mis))


@pytest.mark.parametrize("mis,depth", [(False, 1), (True, 1), (True, 5)])
def test_d3_floor_under_a_constant_map_from_above(mis, depth):
    _closed_form(f"D3 {'PATH_MIS' if mis else 'PATH'} depth {depth}", rg.d3_constant_map(mis, depth))


@pytest.mark.parametrize("mis,depth", [(False, 1), (True, 1), (True, 5)])
def test_d3b_floor_under_a_constant_map_from_below(mis, depth):
    """Back faces: er = 1 / eta, the flipped normal, total internal reflection in the frame's corners."""
    case = rg.d3_constant_map(mis, depth, below=True)
    _, wd = ref.camera_rays(case[0], ref._midpoints())
    assert (np.abs(wd[..., 1]).min(axis=1) < np.sqrt(1 - (1 / rg.ETA) ** 2)).mean() > 0.05, "pixels past the critical angle"
    film = _closed_form(f"D3b {'PATH_MIS' if mis else 'PATH'} depth {depth}", case)
    # with er not inverted the film would have D3's expectation, far outside the tolerance
    wrong = rg.d3_constant_map(mis, depth, below=True, invert=False)
    assert not ref.passes(ref.compare(film, wrong[-3], case[-2], case[-1], SPP))


@pytest.mark.parametrize("mis", [False, True])
def test_d4_emitter_below_the_rough_glass_floor(mis):
    """The transmission lobe's shape against Walter's formula; the emitter hit counted in full under both integrators."""
    _closed_form(f"D4 {'PATH_MIS' if mis else 'PATH'}", rg.d4_emitter_below(mis))


def _part(name, film, mu, vmax, mask):
    rows = ref.compare(film, mu, vmax, mask, SPP)
    print(f"{name}: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), name
    for k in (1.03, 0.97):
        assert not ref.passes(ref.compare(film, mu * k, vmax, mask, SPP)), f"{name}: mu x {k} passes too"


def test_d5_gold_glass_and_grey_in_one_level_3_pass():
    """Level 3 running all three rough materials: the frame, and each part under its own bound of one sample.  The gold
    part pins ggx_eval_h, the lights' wo.h in the record and k_path_nee<.., 3>'s conductor branch; the grey part its
    kind-1 tail."""
    cfg, mu, vmax, include, parts = rg.d5_three_materials()
    g = Renderer(cfg)
    try:
        film = g.render_pass(0, SPP)
        n3 = g.roughglass_launches()
        assert n3 > 0 and g.rough_launches() == n3 and g.conductor_launches() == n3 and g.octree()["depth"] > 0
    finally:
        g.close()
    _part("D5 frame", film, mu, vmax, include)
    for name, (mask, vpart) in parts.items():
        _part(f"D5 {name}", film, mu, vpart, mask)
    # the parts differ by more than any tolerance: the glass is no grey and no gold
    m_gl, m_gr = parts["glass"][0], parts["grey"][0]
    assert mu[m_gr].mean() > 5 * mu[m_gl].mean()


@pytest.mark.parametrize("mis", [False, True])
def test_d6_floor_under_the_map_seen_in_a_mirror_wall(mis):
    """D3 with G4's mirror wall, depth 2: incoming beta != 1 and prevPdf = 0 ahead of a rough-glass vertex, both of its
    branches behind a mirror, the wall hiding part of the sky from NEE and handing it back through the bounce, classes
    0 and 1 in one level-3 pass.  The whole frame, and under PATH_MIS the mirror image alone (its tolerance is 2.7 % of
    its mean there and 6.7 % under PATH: it is held to mu and must fail without the mirror's R = 0.9, 11 % brighter)."""
    cfg, env, mu, vmax, include, seen_mirror = rg.d6_map_mirror(mis)
    film = _closed_form(f"D6 {'PATH_MIS' if mis else 'PATH'}", (cfg, env, mu, vmax, include), multi_level=True)
    if mis:
        rows = ref.compare(film, mu, vmax, seen_mirror, SPP)
        print(f"D6 mirror image alone: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
        assert ref.passes(rows)
        assert not ref.passes(ref.compare(film, mu / rr.G4_R, vmax, seen_mirror, SPP))


def test_d6d_glass_floor_under_the_distant_light_seen_in_a_mirror_wall():
    """The same wall under D1's distant light, where the mirror image alone can be held to +-3 %: k_path_nee's x = beta
    with an incoming beta of 0.9."""
    cfg, mu, vmax, include, seen_mirror = rg.d6_mirror_wall()
    film = _closed_form("D6d", (cfg, mu, vmax, include), multi_level=True)
    _part("D6d mirror image alone", film, mu, vmax, seen_mirror)
    # without the mirror's R = 0.9 the mirror image alone would be 11 % too bright
    assert not ref.passes(ref.compare(film, mu / rr.G4_R, vmax, seen_mirror, SPP))


# ------------------------------------------------------------------------------------------ 5. split passes, albedo

@pytest.mark.parametrize("which", ["d1", "d1_multi", "d3"])
def test_split_passes_give_one_pass_bits(which):
    case = {"d1": lambda: rg.d1_distant(0.5), "d1_multi": lambda: rg.d1_distant(0.2, True),
            "d3": lambda: rg.d3_constant_map(True, 5)}[which]()
    env = case[1] if len(case) == 5 else None
    one = _render(case[0], env)[0]
    two = _render(case[0], env, spans=((0, 128), (128, 256)))[0]
    assert np.array_equal(bits(one), bits(two))


def test_albedo_film_is_one_on_rough_glass():
    """rt_render_features_albedo leaves rough glass un-demodulated: every camera ray hits the floor, so each pixel holds
    k (1, 1, 1, 1) summed in index order."""
    cfg = rg.d1_distant(0.5)[0]
    g = Renderer(cfg)
    try:
        _, _, alb = g.render_features_albedo(0, 3)
    finally:
        g.close()
    one = np.ones(4, f32)
    want = (one + one) + one
    assert np.array_equal(bits(alb), bits(np.broadcast_to(want, alb.shape)))
