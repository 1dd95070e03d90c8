"""Compacted closest hits of the single-leaf simple path (RTMI_HIT_COMPACT): at depths >= 1 the trace
appends one record per hit to a dense hit queue and the shade runs only those.  Per-slot arithmetic and its order are
unchanged, so every film below equals the oracle's bit for bit (tolerance 0) with the knob off and on, and the two
runs' rt_stats are equal field by field."""
import numpy as np
import pytest

from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_oracle_films = {}


def oracle_film(oracle_lib, key, cfg, n):
    """The oracle's film of indices [0, n), computed once per scene (key) and shared by the knob-off and knob-on
    cases; callers only read it."""
    if key not in _oracle_films:
        f = oracle_lib.OracleScene(cfg).render(0, n)
        f.setflags(write=False)
        _oracle_films[key] = f
    return _oracle_films[key]


def counts(st):
    """rt_stats without the stage times."""
    return {k: v for k, v in st.items() if not k.startswith("ms_")}


def render(monkeypatch, cfg, n, knob, env=()):
    monkeypatch.setenv("RTMI_HIT_COMPACT", str(knob))
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    g = Renderer(cfg)
    film = g.render_pass(0, n)
    st = counts(g.stats())
    g.close()
    return film, st


def floor_and_light():
    """One floor quad (2 triangles) and a quad light 300 above it that exists only as a light, not as geometry: a
    bounce ray leaves the floor upwards and nothing is there to hit, so every ray of depth >= 1 misses."""
    P = lambda *v: np.array(v, float)
    faces = np.array([(P(0, 0, 0), P(0, 0, 560), P(550, 0, 560)), (P(0, 0, 0), P(550, 0, 560), P(550, 0, 0))])
    pos, nrm, idx = scene._flat_mesh(faces[:, :, [0, 2, 1]])  # object space: y and z swapped (cornell_box)
    light = dict(p=(343.0, 300.0, 227.0), e1=(0.0, 0.0, 105.0), e2=(-130.0, 0.0, 0.0), n=(0.0, -1.0, 0.0), material=1)
    return scene.TriModel(pos, nrm, idx, rigid=np.eye(4), cull_backfaces=False, octree_capacity=40,
                          tri_material=np.zeros(2, np.int32),
                          materials=[(scene.CORNELL_WHITE, 0.0), ((0.0, 0.0, 0.0), scene.CORNELL_LIGHT_SCALE)],
                          lights=[light])


@pytest.mark.parametrize("knob", [0, 1])
def test_ragged_chunks_two_lanes(oracle_lib, monkeypatch, knob):
    """851 pixels, 2 indices per batch on two lanes, 7 indices: queue and hit-queue lengths are no multiples of the
    512-item chunk, the last chunks are partial, the batch count (4) leaves the last lane group half empty, and the
    counter regions ping-pong over four bounce depths and two batches per lane."""
    cfg = scene.cfg_cornell(res=(37, 23), spp_side=3)
    fo = oracle_film(oracle_lib, "ragged", cfg, 7)
    fg, _ = render(monkeypatch, cfg, 7, knob, [("RTMI_BATCH_SAMPLES", 37 * 23 * 2), ("RTMI_LANES", 2)])
    bad = np.any(bits(fg) != bits(fo), axis=1)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ; max |diff| {np.abs(fg - fo).max()}"


@pytest.mark.parametrize("knob", [0, 1])
@pytest.mark.parametrize("max_depth", [1, 2, 5])
def test_depth_edges(oracle_lib, monkeypatch, max_depth, knob):
    """max_depth 1: no bounce trace at all; 2: one compacted depth, which is also the last (its shade draws no bounce);
    5: the benchmark's."""
    cfg = scene.cfg_cornell(res=(48, 40), spp_side=2, max_depth=max_depth)
    fo = oracle_film(oracle_lib, ("depth", max_depth), cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    assert st["launches_trace"] == max(1, max_depth)


@pytest.mark.parametrize("knob", [0, 1])
def test_all_bounce_rays_miss(oracle_lib, monkeypatch, knob):
    """Every ray of depth >= 1 misses: the hit queues are empty (zero-item shade launches), and the film still
    carries the depth-0 NEE."""
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=40.0, position=(278.0, 400.0, -300.0),
                                  look=(0.0, -0.6, 0.8), right=(1, 0, 0), worldup=(0, 1, 0), res=(40, 24),
                                  lens_radius=0.0, focal_distance=0.0, aspect_fix=True)
    cfg = scene.Config("floor_light", floor_and_light(), cam, scene.StratifiedSampler(2, 2, True, 0),
                       scene.Film(res=(40, 24), filter=capi.RT_FILTER_BOX),
                       scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=4), 0, 4)
    fo = oracle_film(oracle_lib, "floor", cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    assert fo[:, :3].max() > 0                  # the floor is lit
    assert st["rays"] > st["samples"]           # bounce rays were traced ...
    assert 0 < st["hits"] <= st["samples"]      # ... and only camera rays hit anything
    assert st["launches_shade"] == 4


@pytest.mark.parametrize("knob", [0, 1])
def test_camera_misses_at_depth0(oracle_lib, monkeypatch, knob):
    """A wide view from the Cornell eye point: the frame's border looks past the box, those pixels' L is exactly 0
    (the lean depth 0 writes it for the camera misses) and the film equals the oracle's."""
    res = (44, 36)
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=100.0, position=(278.0, 273.0, -800.0), look=(0, 0, 1),
                                  right=(1, 0, 0), worldup=(0, 1, 0), res=res, lens_radius=0.0, focal_distance=0.0,
                                  aspect_fix=True)
    cfg = scene.Config("cornell_wide", scene.cornell_box(), cam, scene.StratifiedSampler(2, 2, True, 0),
                       scene.Film(res=res, filter=capi.RT_FILTER_BOX),
                       scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=5), 0, 4)
    fo = oracle_film(oracle_lib, "wide", cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    dark = np.all(fg[:, :3] == 0, axis=1)
    assert dark[0] and dark[-1] and 0.05 < dark.mean() < 1      # the corners see nothing, the centre sees the box
    assert st["hits"] < st["rays"]


def test_stats_equal_knob_off_and_on(monkeypatch):
    """rt_stats (rays, hits, shadow rays, triangle and node tests, launches ...) do not depend on the knob."""
    cfg = scene.cfg_cornell(res=(64, 64), spp_side=4)
    f0, s0 = render(monkeypatch, cfg, 16, 0)
    f1, s1 = render(monkeypatch, cfg, 16, 1)
    assert s0 == s1
    assert s0["hits"] < s0["rays"] and s0["shadow_rays"] > 0
    assert np.array_equal(bits(f0), bits(f1))
