"""Which traversal instantiation the closed-form scenes of the newer features select ("Instantiation
families"), decided on the CPU from the oracle's octree.

The host picks QCAP from the exact worst case of the BFS group FIFO (rt_host.cpp octree_limits): a single leaf runs
QCAP 1, a bound of at most 16 groups the register FIFO (QCAP 16), a larger one the LDS + HBM ring (QCAP 0, which
runs without a fallback launch while the bound is at most kCoopFifo = 2048).  The "tessellated" floor of the film
tests, 48 x 48 x 2 triangles, has a bound of 64 or 128: QCAP 0.  This file pins that, and pins a coarser floor
(12 x 12 cells) whose bound is at most 16, for tests/test_gpu_instantiations.py to render through QCAP 16.  The closed
forms are of the plane, not of its triangles: mu, vmax and include of the coarse floor are the fine floor's bits.

SCENES is shared with tests/test_gpu_instantiations.py: every scene it renders, at both floors.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import envlight_reference as er
import medium_reference as md
import meshlight_reference as ml
import metal_reference as mr
import radiometry_reference as ref
import rough_reference as rr
import roughglass_reference as rg
import texture_reference as tr

REGISTER_FIFO = 16          # rt_host.cpp octree_limits: caps[] = {16}
COOP_FIFO = 2048            # rt_internal.h kCoopFifo

# cfg, env (scene.Environment or None), media (list or None), mu, vmax, include, extra (what the builder returns beyond)
Case = namedtuple("Case", "cfg env media mu vmax include extra")


def _plain(c):
    return Case(c[0], None, None, c[1], c[2], c[3], c[4:])


def _with_env(c):
    return Case(c[0], c[1], None, c[2], c[3], c[4], c[5:])


def _with_media(c):
    return Case(c[0], None, c[1], c[2], c[3], c[4], c[5:])


def e7_coeffs():
    """The sigmoid of E7's grey texel by the host's rt_rgb_to_sigmoid (the device's bake is pinned to it elsewhere)."""
    return tuple(float(v) for v in tr.rgb8_sigmoid(np.full((1, 3), er.E7_GREY, np.uint8))[0])


# name -> builder(tessellated, **kw) -> Case.  The parameters are those of tests/test_gpu_instantiations.py's table.
BUILDERS = {
    "g1": lambda t: _plain(rr.g1_distant(0.2, t)),
    "g4": lambda t: _plain(rr.g4_mirror(tessellated=t)),
    "g6": lambda t: _plain(rr.g1_distant(0.5, t, texture=True)),
    "m1": lambda t: _plain(mr.m1_distant("Au", 0.2, t)),
    "d1": lambda t: _plain(rg.d1_distant(0.2, t)),
    "d5": lambda t: _plain(rg.d5_three_materials(tessellated=t)),
    "d6": lambda t: _with_env(rg.d6_map_mirror(True, tessellated=t)),
    "ml1": lambda t: _plain(ml.ml1(True, 5, t)),
    "e1": lambda t: _with_env(er.e1(True, 5, t)),
    "e7": lambda t, co=None: _with_env(er.e7(e7_coeffs() if co is None else co, t)),
    "slab": lambda t: _with_media(md.m1_slab(t)),
}

# The table: scene -> (n of the coarse floor, its octree depth, its FIFO bound, the FIFO bound of the 48-floor), as the
# oracle's octree gives them.  n = 12 keeps every scene at or below 16 groups: no scene needed a smaller n.  The wall
# (g4, d6) and the lamp (ml1) enlarge the root box, which halves the bounds; the slab's two faces do not change them.
# d5's coarse floor has 13 columns: the seam at D5_EDGE is a cell edge of the 48-floor only (ref._floor_tris x_lines).
SCENES = {
    "g1": (12, 3, 8, 128),
    "g4": (12, 3, 4, 64),
    "g6": (12, 3, 8, 128),
    "m1": (12, 3, 8, 128),
    "d1": (12, 3, 8, 128),
    "d5": (12, 3, 8, 128),
    "d6": (12, 3, 4, 64),
    "ml1": (12, 3, 4, 64),
    "e1": (12, 3, 8, 128),
    "e7": (12, 3, 8, 128),
    "slab": (12, 3, 8, 128),
}
assert set(SCENES) == set(BUILDERS)


@functools.lru_cache(maxsize=None)
def scene_case(name, fine, co=None):
    """The Case of a scene at the fine floor (True) or at its coarse one; computed once, shared, not to be modified."""
    t = True if fine else SCENES[name][0]
    case = BUILDERS[name](t) if co is None else BUILDERS[name](t, co)
    for a in (case.mu, case.vmax, case.include):
        a.setflags(write=False)
    return case


def fifo_bound(child):
    """The cooperative BFS's FIFO with every box test passing, the loop of test_gpu_bvh.py's _coop_push_replay and of
    rt_host.cpp's octree_limits: the largest number of queued groups right after a push."""
    q, head, worst = [], 0, 0
    if child[0] >= 0:
        q.append(int(child[0]))
        worst = 1
    while head < len(q):
        g = q[head]
        head += 1
        for i in range(8):
            c = int(child[g + i])
            if c >= 0:
                q.append(c)
                worst = max(worst, len(q) - head)
    return worst


def _same_model(a, b):
    ma, mb = a.cfg.model, b.cfg.model
    for k in ("positions", "normals", "indices", "tri_material"):
        x, y = np.asarray(getattr(ma, k)), np.asarray(getattr(mb, k))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert repr(ma.materials) == repr(mb.materials) and repr(ma.lights) == repr(mb.lights)
    assert (a.cfg.name, a.cfg.index_begin, a.cfg.index_end) == (b.cfg.name, b.cfg.index_begin, b.cfg.index_end)
    assert bytes(a.cfg.integrator.desc()) == bytes(b.cfg.integrator.desc())


def _same_expectation(a, b):
    for k in ("mu", "vmax", "include"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_floor_cells():
    assert ref.floor_cells(False) == 1 and ref.floor_cells(True) == 48 == ref.TESSELLATED_N
    assert ref.floor_cells(np.bool_(True)) == 48 and ref.floor_cells(np.bool_(False)) == 1
    assert [ref.floor_cells(n) for n in (1, 6, 12, 48)] == [1, 6, 12, 48]
    with pytest.raises(AssertionError):
        ref.floor_cells(0)
    assert len(ref._floor_tris(12)) == 288 and len(ref._floor_tris(12, (rg.D5_EDGE,))) == 312
    # a line of the grid adds nothing: D5's seam is a cell edge of the 48-floor
    assert np.array_equal(ref._floor_tris(48, (rg.D5_EDGE, 0.0)), ref._floor_tris(48))


@pytest.mark.parametrize("name", ["g4", "d5", "slab", "ml1"])
def test_todays_cases_are_unchanged(name):
    """The builders' defaults, tessellated=True and tessellated=48 are one scene and one expectation, bit for bit."""
    today = {"g4": lambda: _plain(rr.g4_mirror()), "d5": lambda: _plain(rg.d5_three_materials()),
             "slab": lambda: _with_media(md.m1_slab(True)), "ml1": lambda: _plain(ml.ml1(True, 5, True))}[name]()
    for other in (scene_case(name, True), BUILDERS[name](48)):
        _same_model(today, other)
        _same_expectation(today, other)
    assert len(today.cfg.model.indices) >= 2 * 48 * 48


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_selects_its_fifo(oracle_lib, name):
    """The coarse floor: a multi-level octree whose bound fits the register FIFO (QCAP 16); the fine floor: a bound
    above it and within kCoopFifo (QCAP 0 with coop_ok, no fallback launch); one expectation for both.  Each builder
    asserts vmax < 1 and at most EXCLUDED_MAX excluded pixels on its own inputs (ref._finish)."""
    n, depth, bound, bound48 = SCENES[name]
    coarse, fine = scene_case(name, False), scene_case(name, True)
    oc = oracle_lib.OracleScene(coarse.cfg).octree()
    got = (oc["depth"], fifo_bound(oc["child"]))
    print(f"{name}: n {n}, {len(coarse.cfg.model.indices)} triangles, depth {got[0]}, bound {got[1]}")
    assert got == (depth, bound)
    assert depth > 0 and 1 <= bound <= REGISTER_FIFO
    of = oracle_lib.OracleScene(fine.cfg).octree()
    assert of["depth"] > 0 and fifo_bound(of["child"]) == bound48
    assert REGISTER_FIFO < bound48 <= COOP_FIFO
    _same_expectation(coarse, fine)
    assert np.all(coarse.vmax < 1.0) and 1.0 - coarse.include.mean() <= ref.EXCLUDED_MAX
    assert len(coarse.cfg.model.indices) < len(fine.cfg.model.indices)
    if name == "d5":            # the parts' masks and bounds too
        for k, (mask, vpart) in coarse.extra[0].items():
            assert np.array_equal(mask, fine.extra[0][k][0]) and np.array_equal(vpart, fine.extra[0][k][1])
    if name in ("g4", "d6"):
        assert np.array_equal(coarse.extra[0], fine.extra[0])
