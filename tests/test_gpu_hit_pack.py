"""Packed hit records of the single-leaf simple path (RTMI_HIT_PACK): at depths >= 1 the trace writes one
float4 per hit, (b0, b1, b2, slot | prim << 24 | facing << 30), the facing bit formed with the shade's own expression,
and the shade takes the face normal from LDS; at depth 0 the w lane of hitB is prim | front << 29 | flip << 30 (-1 for
a miss) and the shade reads neither hitPrim nor the ray.  Per-slot arithmetic and its order are unchanged, so every film below
equals the oracle's (or the unpacked path's, where the oracle is too slow) bit for bit, tolerance 0, with the knob off
and on, and rt_stats are equal field by field."""
import dataclasses

import numpy as np
import pytest

import denoise_reference as dref
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import Renderer, records_to_arrays

gpu = pytest.mark.gpu  # (the facing census below runs on the CPU)


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
    monkeypatch.setenv("RTMI_HIT_PACK", str(knob))
    for k, v in env:
        monkeypatch.setenv(k, str(v))
    g = Renderer(cfg)
    film = g.render_pass(0, n)
    st = counts(g.stats())
    g.close()
    return film, st


def wide_camera(res):
    """The Cornell eye point with fov 100: the frame's border looks past the box."""
    return scene.PerspectiveCamera(near=1.0, far=5000.0, fov=100.0, position=(278.0, 273.0, -800.0), look=(0, 0, 1),
                                   right=(1, 0, 0), worldup=(0, 1, 0), res=res, lens_radius=0.0, focal_distance=0.0,
                                   aspect_fix=True)


def cornell_cfg(model, res, cam=None, max_depth=5):
    return scene.Config("cornell_pack", model, cam or scene.cornell_camera(res), scene.StratifiedSampler(2, 2, True, 0),
                        scene.Film(res=res, filter=capi.RT_FILTER_BOX),
                        scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=max_depth), 0, 4)


def reversed_block_box():
    """The Cornell box with the winding of the short block's 12 triangles and of the light's 2 reversed (their face
    normals point into the block / up), back faces not culled: rays that see the block or the light look at the back
    of its triangles, and the camera rays that hit the emitter add no Le (the quad light itself is unchanged)."""
    m = scene.cornell_box()
    faces = np.asarray(m.positions, np.float64).reshape(-1, 3, 3).copy()
    faces[10:24] = faces[10:24][:, [0, 2, 1]]
    pos, nrm, idx = scene._flat_mesh(faces)
    return dataclasses.replace(m, positions=pos, normals=nrm, indices=idx, cull_backfaces=False)


def blob_box():
    """The block-less Cornell box (12 triangles) with an 80-triangle blob on its floor, in one leaf: more triangles
    than the LDS triangle table or a packed record's prim field holds."""
    pos, _, idx = scene.procedural_blob(frequency=2, radius=1.0, seed=1)
    tri = pos[idx].astype(np.float64)
    lo = tri.reshape(-1, 3).min(0)
    world = tri * 150.0 + np.array([278.0, -lo[1] * 150.0 + 0.5, 280.0])
    m = scene.cornell_box(blocks=False, extra=world)
    return dataclasses.replace(m, octree_capacity=200)


@gpu
@pytest.mark.parametrize("knob", [0, 1])
def test_ragged_chunks_two_lanes(oracle_lib, monkeypatch, knob):
    """851 pixels, 2 indices per batch on two lanes, 7 indices: queue and hit-queue lengths are no multiples of the
    512-item chunk, the last chunks are partial and the last lane group is half empty."""
    cfg = scene.cfg_cornell(res=(37, 23), spp_side=3)
    fo = oracle_film(oracle_lib, "ragged", cfg, 7)
    fg, _ = render(monkeypatch, cfg, 7, knob, [("RTMI_BATCH_SAMPLES", 37 * 23 * 2), ("RTMI_LANES", 2)])
    bad = np.any(bits(fg) != bits(fo), axis=1)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ; max |diff| {np.abs(fg - fo).max()}"


@gpu
@pytest.mark.parametrize("knob", [0, 1])
@pytest.mark.parametrize("max_depth", [1, 2, 5])
def test_depth_edges(oracle_lib, monkeypatch, max_depth, knob):
    """max_depth 1: no packed depth at all; 2: one packed depth, which is also the last (its shade draws no bounce);
    5: the benchmark's."""
    cfg = scene.cfg_cornell(res=(48, 40), spp_side=2, max_depth=max_depth)
    fo = oracle_film(oracle_lib, ("depth", max_depth), cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    assert st["launches_trace"] == max(1, max_depth)


@gpu
@pytest.mark.parametrize("knob", [0, 1])
def test_camera_misses(oracle_lib, monkeypatch, knob):
    """The wide view: the border pixels' camera rays miss, their L is exactly 0, and bounce rays leave the box through
    its open front (misses at the packed depths)."""
    res = (44, 36)
    cfg = cornell_cfg(scene.cornell_box(), res, wide_camera(res))
    fo = oracle_film(oracle_lib, "wide", cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    dark = np.all(fg[:, :3] == 0, axis=1)
    assert dark[0] and dark[-1] and 0.05 < dark.mean() < 1
    assert st["hits"] < st["rays"]


def test_reversed_block_has_both_facings(oracle_lib):
    """CPU: among the first hits of the reversed-block scene, the predicate the facing bit carries, dot(face normal,
    normalised direction) > 0 in float32 as the kernels order it, takes both values (the plain Cornell box has only
    front-face hits), so a wrong bit changes the film of the next test."""
    res = (48, 40)
    cfg = cornell_cfg(reversed_block_box(), res)
    n = res[0] * res[1]
    r = records_to_arrays(oracle_lib.OracleScene(dref.record_config(cfg)).samples(np.arange(n, dtype=np.int32),
                                                                                  np.zeros(n, np.int32)))
    prim = np.asarray(r["prim"])
    hit = prim >= 0
    F = np.float32
    # world space = object space with y and z swapped (ObjectToRender = the permutation alone)
    tri = np.asarray(cfg.model.positions, F)[np.asarray(cfg.model.indices, np.int64)][:, :, [0, 2, 1]]
    a, b = tri[:, 0] - tri[:, 2], tri[:, 1] - tri[:, 2]
    cr = np.stack([a[:, 1] * b[:, 2] - b[:, 1] * a[:, 2], a[:, 2] * b[:, 0] - b[:, 2] * a[:, 0],
                   a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]], axis=1).astype(F)

    def norm(v):
        s = F(1) / np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2], dtype=F)
        return (v * s[:, None]).astype(F)
    ng, d = norm(cr)[prim[hit]], norm(np.asarray(r["rd"], F)[hit])
    facing = (ng[:, 0] * d[:, 0] + ng[:, 1] * d[:, 1]) + ng[:, 2] * d[:, 2] > 0
    assert facing.sum() > 20 and (~facing).sum() > 20
    assert np.all((prim[hit][facing] >= 10) & (prim[hit][facing] < 24))  # the reversed triangles, and nothing else
    assert np.any(prim[hit][facing] < 12) and np.any(prim[hit][facing] >= 12)  # the emitter's back and the block's


@gpu
@pytest.mark.parametrize("knob", [0, 1])
def test_both_facing_values(oracle_lib, monkeypatch, knob):
    """The reversed-block scene against the oracle: hits with the facing bit set (the shade flips the staged normal)
    and clear, at depth 0 (where the emitter is seen from behind: the front bit clear) and at the packed depths."""
    cfg = cornell_cfg(reversed_block_box(), (48, 40))
    fo = oracle_film(oracle_lib, "reversed", cfg, 4)
    fg, _ = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))


@gpu
def test_stats_equal_knob_off_and_on(monkeypatch):
    """rt_stats (rays, hits, shadow rays, triangle and node tests, launches ...) do not depend on the knob.  Cornell's
    triangle ids reach 35, so bit 5 of the record's prim field is in use."""
    cfg = scene.cfg_cornell(res=(64, 64), spp_side=4)
    f0, s0 = render(monkeypatch, cfg, 16, 0)
    f1, s1 = render(monkeypatch, cfg, 16, 1)
    assert s0 == s1
    assert s0["hits"] < s0["rays"] and s0["shadow_rays"] > 0
    assert np.array_equal(bits(f0), bits(f1))


@gpu
def test_slot_field_at_its_limit(monkeypatch):
    """One batch of exactly 2^24 samples: slots reach 2^24 - 1, every bit of the record's slot field.  Knob 0 (pinned
    to the oracle by the cases above) against knob 1; the oracle is too slow at this size."""
    cfg = scene.cfg_cornell(res=(4096, 4096), spp_side=1)
    f0, s0 = render(monkeypatch, cfg, 1, 0, [("RTMI_LANES", 1)])
    f1, s1 = render(monkeypatch, cfg, 1, 1, [("RTMI_LANES", 1)])
    assert s0["samples"] == 1 << 24 and s0 == s1
    assert np.array_equal(bits(f0), bits(f1))


@gpu
def test_oversize_batch_is_not_packed(monkeypatch):
    """A batch above 2^24 samples: a slot no longer fits the record, so the unpacked path runs whatever the knob says
    (packed, the high slots would alias low ones and the films would differ)."""
    n = 4100 * 4100
    cfg = scene.cfg_cornell(res=(4100, 4100), spp_side=1)
    env = [("RTMI_LANES", 1), ("RTMI_BATCH_SAMPLES", n)]
    f0, s0 = render(monkeypatch, cfg, 1, 0, env)
    f1, s1 = render(monkeypatch, cfg, 1, 1, env)
    assert s0["samples"] == n and s0 == s1
    assert s0["launches_trace"] == 5            # one batch: a launch per depth
    assert np.array_equal(bits(f0), bits(f1))


@gpu
@pytest.mark.parametrize("knob", [0, 1])
def test_more_than_64_triangles_in_one_leaf(oracle_lib, monkeypatch, knob):
    """92 triangles in a single leaf: neither the LDS triangle table nor the prim field holds them, the unpacked
    records run and the film equals the oracle's."""
    cfg = cornell_cfg(blob_box(), (40, 32))
    assert len(cfg.model.indices) == 92
    oc = oracle_lib.OracleScene(cfg).octree()
    assert len(oc["child"]) == 1 and oc["leaf_count"][0] == 92      # one node, a leaf with every triangle
    fo = oracle_film(oracle_lib, "blob", cfg, 4)
    fg, st = render(monkeypatch, cfg, 4, knob)
    assert np.array_equal(bits(fg), bits(fo))
    assert st["hits"] < st["rays"]
