"""Absorbing media inside glass on the device: the stage's transmittance function bit for bit against
tests/medium_reference.py, rt_scene_set_media's validation and lifecycle, neutrality without a medium, determinism across
split passes and lanes, the segment counter, and the films M1 (four variants), M2 (grey and red) and M3 (PATH_MIS depth 5,
PATH depth 2) against float64 closed forms with radiometry_reference.tolerance.  The measured |got - mu| / tol of each is
recorded in DESIGN.md §3n.

Not here: the issue's "stage against restatement" film (M1 at 1 spp reassembled from the debug sample records).  The
records (rt_sample_record) hold the camera segment only - ro, rd, the first hit's prim, b, t - and the final L; the
attenuated segment is the second one, whose float32 length t |d| starts at the shade's offset point and is exposed
nowhere, so the per-sample factor cannot be formed from them bit for bit.  The device function is pinned bit for bit
below, and what the stage does with it by the closed-form films and the exact segment count."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import medium_reference as mr
import radiometry_reference as ref
import roughglass_reference as rgr
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
SPP = 256


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1. the device function

def test_device_function_bit_for_bit():
    cfg = ref._config("medium_floor", ref._floor_model(False), ref._down_camera(), 16, capi.RT_INTEGRATOR_PATH, 1,
                      film=ref._film())
    g = Renderer(cfg)
    try:
        for name, c, sigma, lam, length in mr.items(4096):
            got = g.medium_eval(mr.media_of(c, sigma), lam, length)
            want = mr.transmittance32(c, sigma, lam, length)
            x = mr.exponent32(c, sigma, lam, length)
            assert not np.any(mr.near_midpoint64(x[x < mr.CUT])), name
            assert np.array_equal(bits(got), bits(want)), f"{name}: {np.sum(bits(got) != bits(want))} differ"
            host = scene.medium_transmittance(mr.media_of(c, sigma), lam, length)
            assert np.array_equal(bits(got), bits(host)), name
            assert (got == 0).any() or name == "grey"
            assert (got == 1).sum() >= 64 and ((got > 0) & (got < 1)).sum() > 20000
        F = C.POINTER(C.c_float)
        m = scene.media_array([scene.Medium(mr.GREY, 1.0)])
        lam, ln, out = np.full(8, 500.0, f32), np.ones(1, f32), np.zeros(8, f32)
        p = lambda a: a.ctypes.data_as(F)
        assert g.lib.rt_debug_medium_eval(g.h, m, 0, None, None, None) == capi.RT_OK
        assert g.lib.rt_debug_medium_eval(g.h, m, -1, p(lam), p(ln), p(out)) == capi.RT_E_ARG
        assert g.lib.rt_debug_medium_eval(g.h, None, 1, p(lam), p(ln), p(out)) == capi.RT_E_ARG
        assert g.lib.rt_debug_medium_eval(g.h, m, 1, p(lam), p(ln), None) == capi.RT_E_ARG
        assert g.lib.rt_debug_medium_stats(g.h, None, None) == capi.RT_E_ARG
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 2. validation, lifecycle

def _small_m1(spp=16):
    cfg = mr.m1_slab(False)[0]
    cfg.sampler = scene.StratifiedSampler(4, 4, True, 0)
    cfg.index_end = spp
    return cfg


def _set(g, media):
    arr = scene.media_array(media) if media is not None else None
    rc = g.lib.rt_scene_set_media(g.h, arr, 0 if media is None else len(media))
    return rc, g.lib.rt_last_error(g.h).decode()


def test_validation_keeps_the_media_bound_before():
    g = Renderer(_small_m1())
    try:
        plain = g.render_pass(0, 16)
        assert g.medium_stats() == (0, 0)
        good = [None, scene.Medium(ref.S_GREEN, mr.M1_SIGMA)]
        g.set_media(good)
        before = g.render_pass(0, 16)
        n, seg = g.medium_stats()
        assert n > 0 and seg == 64 * 64 * 16 and not np.array_equal(bits(before), bits(plain))
        inf, nan = float("inf"), float("nan")
        bad = [([None], "n_materials"), ([None, None, None], "n_materials"),
               ([None, scene.Medium(ref.S_GREEN, nan)], "material 1: sigma"),
               ([None, scene.Medium(ref.S_GREEN, inf)], "material 1: sigma"),
               ([None, scene.Medium(ref.S_GREEN, -0.01)], "material 1: sigma"),
               ([scene.Medium(ref.S_GREEN, -1.0), None], "material 0: sigma"),
               ([None, scene.Medium((nan, 0.0, 0.0), 0.01)], "material 1: sigmoid[0]"),
               ([None, scene.Medium((0.0, 0.0, inf), 0.01)], "material 1: sigmoid[2]"),
               ([scene.Medium(mr.GREY, 0.01), None], "material 0: sigma > 0 on an emissive")]
        for media, word in bad:
            rc, msg = _set(g, media)
            assert rc == capi.RT_E_ARG and word in msg, (media, msg)
            assert np.array_equal(bits(g.render_pass(0, 16)), bits(before)), media
            assert g.medium_stats()[1] == seg
        # non-finite coefficients are not read while sigma == 0
        assert _set(g, [scene.Medium((nan, inf, 0.0), 0.0), scene.Medium(ref.S_GREEN, mr.M1_SIGMA)])[0] == capi.RT_OK
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(before))
        # NULL and n == 0 clear; rt_scene_upload drops the media
        assert _set(g, None)[0] == capi.RT_OK
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(plain)) and g.medium_stats() == (0, 0)
        g.set_media(good)
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(before))
        d = g.cfg.model.desc()
        assert g.lib.rt_scene_upload(g.h, C.byref(d)) == capi.RT_OK
        assert np.array_equal(bits(g.render_pass(0, 16)), bits(plain)) and g.medium_stats() == (0, 0)
    finally:
        g.close()


def test_a_material_table_too_large_for_lds_reads_through_the_pointer():
    """More than 256 materials: the stage reads the medium table from global memory.  The padding materials are used by
    no triangle, so the film and the segment count are those of the two-material scene, bit for bit."""
    media = [None, scene.Medium(ref.S_GREEN, mr.M1_SIGMA)]
    films = []
    for pad in (0, 299):
        cfg = _small_m1()
        cfg.model.materials = list(cfg.model.materials) + [(mr.GREY, 0.0)] * pad
        g = Renderer(cfg)
        try:
            g.set_media(media + [None] * pad)
            films.append(g.render_pass(0, 16))
            assert g.medium_stats()[1] == 64 * 64 * 16
        finally:
            g.close()
    assert films[0][:, :3].max() > 0 and np.array_equal(bits(films[0]), bits(films[1]))


def test_only_glass_takes_a_medium():
    """sigma > 0 on a Lambert, mirror, rough or conductor material is refused; on both glasses it binds."""
    cfg = scene.cfg_cornell(res=(32, 32), spp_side=2)
    mats = [tuple(m) for m in cfg.model.materials]
    n = len(mats)
    assert n >= 3
    kinds = {capi.RT_MAT_DIFFUSE: (mr.GREY, 0.0, capi.RT_MAT_DIFFUSE, 0.0),
             capi.RT_MAT_MIRROR: (mr.GREY, 0.0, capi.RT_MAT_MIRROR, 0.0),
             capi.RT_MAT_DIELECTRIC: ((0.0, 0.0, 0.0), 0.0, capi.RT_MAT_DIELECTRIC, 1.5),
             capi.RT_MAT_ROUGH: scene.rough(mr.GREY, 0.3), capi.RT_MAT_CONDUCTOR: scene.metal("Au", 0.3),
             capi.RT_MAT_ROUGH_DIELECTRIC: scene.rough_glass(1.5, 0.3)}
    emit = [i for i, m in enumerate(mats) if m[1] > 0]
    which = [i for i in range(n) if i not in emit][0]
    g = Renderer(cfg)
    try:
        for typ, mat in kinds.items():
            mats2 = list(mats)
            mats2[which] = mat
            cfg.model.materials = mats2
            g.configure(cfg)
            media = [None] * n
            media[which] = scene.Medium(mr.GREY, 0.01)
            rc, msg = _set(g, media)
            ok = typ in (capi.RT_MAT_DIELECTRIC, capi.RT_MAT_ROUGH_DIELECTRIC)
            assert rc == (capi.RT_OK if ok else capi.RT_E_ARG), (typ, msg)
            if not ok:
                assert f"material {which}" in msg and "RT_MAT_DIELECTRIC" in msg
            film = g.render_pass(0, 4)
            assert np.all(np.isfinite(film)) and (g.medium_stats()[0] > 0) == ok
    finally:
        g.close()


def test_state_errors():
    cfg = _small_m1()
    media = [None, scene.Medium(ref.S_GREEN, mr.M1_SIGMA)]
    g = Renderer()
    rc, msg = _set(g, media)
    assert rc == capi.RT_E_STATE and "scene" in msg                      # no scene
    g.configure(cfg)
    g.adaptive_begin(2, 1, 4, 0.0)
    rc, msg = _set(g, media)
    assert rc == capi.RT_E_STATE and "adaptive" in msg
    assert _set(g, None)[0] == capi.RT_E_STATE                            # clearing is refused as well
    g.adaptive_end()
    g.temporal_begin()
    rc, msg = _set(g, media)
    assert rc == capi.RT_E_STATE and "temporal" in msg
    g.temporal_end()
    assert _set(g, media)[0] == capi.RT_OK
    g.close()
    g = Renderer(cfg, device=[0, 0])                                      # a multi-device context (the same device twice)
    rc, msg = _set(g, media)
    assert rc == capi.RT_E_STATE and "one-device" in msg
    g.close()


# ------------------------------------------------------------------------------------------ 3. neutrality

@pytest.mark.parametrize("name", ["cornell", "cfg4", "d1"])
def test_no_medium_launches_nothing_and_keeps_every_bit(name):
    cfg = {"cornell": lambda: scene.cfg_cornell(res=(48, 48), spp_side=2),
           "cfg4": lambda: scene.cfg4_mixed(res=(48, 27), spp=(2, 2), frequency=8),
           "d1": lambda: rgr.d1_distant(0.5)[0]}[name]()
    g = Renderer(cfg)
    try:
        def run():
            film = g.render_pass(0, 4)
            return film, (g.rough_launches(), g.conductor_launches(), g.roughglass_launches()), g.medium_stats()
        film0, launches0, stats0 = run()
        assert stats0 == (0, 0) and film0[:, :3].max() > 0
        n = max(len(cfg.model.materials), 1)
        for media in ([scene.Medium(ref.S_RED, 0.0)] * n, [None] * n, None):
            if media is None:
                g.set_media(None)
            else:
                assert _set(g, media)[0] == capi.RT_OK
            film, launches, stats = run()
            assert stats == (0, 0), (name, stats)
            assert launches == launches0
            assert np.array_equal(bits(film), bits(film0)), name
    finally:
        g.close()


# ------------------------------------------------------------------------------------------ 4. films against float64

def _render(cfg, media, env=None, spans=((0, SPP),)):
    g = Renderer(cfg)
    try:
        if env is not None:
            g.set_environment(env)
        g.set_media(media)
        oc = g.octree()
        depth = oc["depth"], oc["max_queue_groups"]
        film, stats = None, []
        for a, b in spans:
            film = g.render_pass(a, b, film)
            stats.append(g.medium_stats())
        return film, depth, stats
    finally:
        g.close()


def _held(name, film, mu, vmax, include):
    assert np.all(vmax < 1.0)
    rows = ref.compare(film, mu, vmax, include, SPP)
    print(f"\n{name}: |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), name
    for k in (1.03, 0.97):
        assert not ref.passes(ref.compare(film, mu * k, vmax, include, SPP)), f"{name}: mu x {k} passes too"


@pytest.fixture(scope="module")
def m1_tess_film():
    """M1 tessellated, XYZ: one pass over the 256 indices (shared by the film and the determinism tests)."""
    case = mr.m1_slab(True)
    film, depth, stats = _render(case[0], case[1])
    return case, film, depth, stats


@pytest.mark.parametrize("tess,sensor", [(False, "xyz"), (True, "xyz"), (False, "canon_eos_100d"), (True, "canon_eos_100d")])
def test_m1_tilted_slab(tess, sensor, m1_tess_film):
    """Pure Beer-Lambert per wavelength over d / cos theta.  Plain: single leaf, SoA slots; tessellated: multi-level, 128-B
    records, sort and bins.  Exactly one attenuated segment per sample."""
    if tess and sensor == "xyz":
        case, film, depth, stats = m1_tess_film
    else:
        case = mr.m1_slab(tess, sensor, capi.RT_ILLUM_D65 if sensor == "xyz" else capi.RT_ILLUM_A)
        film, depth, stats = _render(case[0], case[1])
    cfg, media, mu, vmax, include, ex = case
    assert (depth[0] > 0) == tess, depth
    assert (depth[1] > 16) == tess, depth   # (QCAP 0 with coop_ok: DESIGN §2)
    launches, segments = stats[-1]
    assert launches > 0 and segments == 64 * 64 * SPP, stats
    name = f"M1 {'tessellated' if tess else 'plain'} {sensor}"
    _held(name, film, mu, vmax, include)
    # the forgotten 1 / cos theta, and absorption as a colour (one Y-weighted mean sigma_a), must both fail
    assert not ref.passes(ref.compare(film, ex["wrong_no_cos"], vmax, include, SPP)), name
    assert not ref.passes(ref.compare(film, ex["wrong_mean_sigma"], vmax, include, SPP)), name


@pytest.mark.parametrize("coloured", [False, True])
def test_m2_sphere_in_a_furnace(coloured):
    """Chords behind refraction: every internal chord of the glass Sphere (an analytic shape: the shape branch of the
    back-face test) ends on a back face and is attenuated, the entry and the exit to the emitter are not."""
    cfg, media, mu, vmax, include, on = mr.m2_sphere(coloured)
    film, _, stats = _render(cfg, media)
    assert stats[-1][0] > 0 and stats[-1][1] > on.sum() * SPP * 0.8     # (a tenth of the samples is reflected at the entry)
    name = f"M2 {'red' if coloured else 'grey'}"
    _held(name, film, mu, vmax, include)
    rows = ref.compare(film, mu, vmax, include & on, SPP)
    print(f"{name}, the sphere alone: |got - mu| / tol = {ref.deviation(rows):.3f}")
    assert ref.passes(rows)
    # without the medium the sphere shows the furnace (K6): far outside
    k6 = ref.k6_furnace("glass")[1]
    assert not ref.passes(ref.compare(film, k6, vmax, include & on, SPP))


@pytest.fixture(scope="module")
def m3_nee():
    return mr.m3_nee_share(mr.M3_ALPHA, 1 / rgr.ETA)[1][0]


@pytest.mark.parametrize("mis,depth", [(True, 5), (False, 2)])
def test_m3_rough_glass_behind_a_window(mis, depth, m3_nee):
    """The stage's placement before the shade: the rough-glass vertex hit from inside carries the attenuation in its NEE
    term as well as in its bounce."""
    cfg, media, env, mu, vmax, include, ex = mr.m3_rough(mis, depth)
    film, _, stats = _render(cfg, media, env)
    assert stats[-1][0] > 0 and stats[-1][1] == 64 * 64 * SPP          # (the floor's back face is met once per sample)
    name = f"M3 {'PATH_MIS' if mis else 'PATH'} depth {depth}"
    _held(name, film, mu, vmax, include)
    if mis:   # the attenuation on the bounce only (the stage after the shade) must fail
        wrong = np.broadcast_to(mr.m3_after_shade(ex, m3_nee), mu.shape)
        assert not ref.passes(ref.compare(film, wrong, vmax, include, SPP)), name


# ------------------------------------------------------------------------------------------ 5. determinism

def test_split_passes_give_one_pass_bits(m1_tess_film):
    case, one, depth, stats = m1_tess_film
    four, _, stats4 = _render(case[0], case[1], spans=((0, 64), (64, 128), (128, 192), (192, 256)))
    assert np.array_equal(bits(one), bits(four))
    assert all(s[0] > 0 and s[1] == 64 * 64 * 64 for s in stats4), stats4


def test_one_lane_gives_the_same_bits(m1_tess_film, tmp_path):
    """A second renderer with RTMI_LANES=1 (read once per context: a child process), small batches in both so that the
    default build runs two lanes."""
    case, one, _, _ = m1_tess_film
    out = tmp_path / "film.npy"
    code = ("import sys\n"
            f"sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})\n"
            "import numpy as np\n"
            "import medium_reference as mr\n"
            "from computational_ray_tracer_amd.renderer import Renderer\n"
            "case = mr.m1_slab(True)\n"
            "g = Renderer(case[0])\n"
            "g.set_media(case[1])\n"
            "film = g.render_pass(0, 256)\n"
            "print('STATS', *g.medium_stats())\n"
            f"np.save({str(out)!r}, film)\n"
            "g.close()\n")
    films = {}
    for lanes in ("1", "2"):
        env = dict(os.environ, RTMI_LANES=lanes, RTMI_BATCH_SAMPLES=str(64 * 64 * 32))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = [l for l in r.stdout.splitlines() if l.startswith("STATS")][0].split()
        assert int(line[1]) > 0 and int(line[2]) == 64 * 64 * 256, line
        films[lanes] = np.load(out)
    assert np.array_equal(bits(films["1"]), bits(one)) and np.array_equal(bits(films["2"]), bits(one))
