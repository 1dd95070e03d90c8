"""GPU: Renderer.trace and Renderer.occluded against float64 brute force (tests/geometry_reference.py), directly.

Every other geometric GPU test compares the kernels with the oracle bit for bit; the oracle restates the same
algorithms in float32, so a defect shared by both sides passes them.  Here the kernels answer to the float64
reference of tests/test_geometry_reference.py themselves: the same scenes, rays, comparator, bounds and caps (case(),
check_trace), no oracle in between.  One test per path a ray can take, with the path asserted from stats():
  * the Cornell box: one leaf, the nearest-first single-leaf kernel;
  * blob8 on the device-built octree (the default upload): the per-thread BVH walk of the debug entry;
  * blob8 on the host-built octree with RTMI_DEBUG_PATH_KERNELS=1: path mode's trace kernel (wave tickets);
  * blob8 with RTMI_FORCE_AMB=2: a quarter of the rays declared ambiguous, carried by the cooperative BFS
    (RTMI_COOP=1) or by k_trace_fallback (RTMI_COOP=0);
  * CFG0 with back-face culling (tile set 1);
  * the shapes scene: closest hit and occlusion through the analytic shapes under rotation and non-uniform scale.
Ray counts are no multiples of 64; one ray alone is traced as well.
"""
import numpy as np
import pytest

import geometry_reference as gr
from computational_ray_tracer_amd import capi
from computational_ray_tracer_amd.renderer import Renderer
from test_geometry_reference import case, check_trace

pytestmark = pytest.mark.gpu


def _check(c, g, forced=False):
    n = len(c.ro)
    assert n % 64 and n % 256
    g.reset_stats()
    prim, bt = g.trace(c.ro, c.rd, c.use_cull)
    rep = check_trace(c, prim, bt)
    print(f"\n{c.name}: {rep.n} rays, undecided {rep.undecided_share:.4f}, |dt| {rep.tri_t_w:.3g} W, bary "
          f"{rep.tri_bary:.3g}, shape t {rep.shape_t}, shape p {rep.shape_p}")
    assert rep.ok, rep.failures
    st = g.stats()
    assert st["rays"] >= n and st["coop_overflows"] == 0, st
    # forced: a quarter of the rays go to the exact fallback.  Otherwise the BVH walk decides nearly every ray itself;
    # only rays from 1e5 away are undecided by design (their origin lies beyond the validity of the BVH's padding)
    far = int((np.abs(c.ro).max(1) > 5e4).sum())
    assert (st["fallback_rays"] > 0.1 * n) if forced else (st["fallback_rays"] <= far + 0.02 * n), st
    occ = g.occluded(c.ro, c.rd, c.tmax)
    fails = gr.compare_occluded(c.occ, occ)
    assert not fails, fails
    assert g.stats()["coop_overflows"] == 0
    # one ray alone: a decided hit
    i = int(np.flatnonzero(c.ref.decided & (c.ref.prim >= 0) & c.ref_all.decided)[0])
    p1, b1 = g.trace(c.ro[i:i + 1], c.rd[i:i + 1], c.use_cull)
    one = c.sref.closest(c.ro[i:i + 1], c.rd[i:i + 1], c.skip)
    rep1 = gr.compare_closest(one, p1, b1, bounds=gr.bounds(c.name))
    assert rep1.ok and one.decided[0] and p1[0] == c.ref.prim[i], rep1.failures
    t1 = np.float32([c.ref_all.t[i] * 2 if np.isfinite(c.ref_all.t[i]) else 400.0])
    want = c.sref.occluded(c.sref.closest(c.ro[i:i + 1], c.rd[i:i + 1]), t1)
    assert want[0] == 1 and g.occluded(c.ro[i:i + 1], c.rd[i:i + 1], t1)[0] == 1


def test_cornell_single_leaf():
    c = case("cornell")
    g = Renderer(c.cfg)
    oc = g.octree()
    assert len(oc["child"]) == 1 and oc["leaf_count"][0] == 36
    _check(c, g)


def test_blob8_device_octree():
    c = case("blob8")
    g = Renderer(c.cfg)                                          # the default upload: the device-built octree
    oc = g.octree()
    assert oc["depth"] >= 2 and len(oc["child"]) == 353
    _check(c, g)


def test_blob8_host_octree_path_kernels(monkeypatch):
    monkeypatch.setenv("RTMI_DEBUG_PATH_KERNELS", "1")
    c = case("blob8")
    g = Renderer(c.cfg, octree_build=capi.RT_OCTREE_BUILD_HOST)
    assert g.octree()["depth"] >= 2
    _check(c, g)


@pytest.mark.parametrize("coop", ["1", "0"])
def test_blob8_forced_fallbacks(monkeypatch, coop):
    """coop 1: the wave-cooperative BFS inside the trace kernel; coop 0: k_trace_fallback after it."""
    monkeypatch.setenv("RTMI_DEBUG_PATH_KERNELS", "1")
    monkeypatch.setenv("RTMI_FORCE_AMB", "2")
    monkeypatch.setenv("RTMI_COOP", coop)
    c = case("blob8")
    _check(c, Renderer(c.cfg), forced=True)


def test_cfg0_culled():
    c = case("cfg0")
    g = Renderer(c.cfg)
    assert g.octree()["depth"] >= 2
    # without the culled tile set the answers differ on many rays, so the comparison sees which set ran
    assert (c.ref.prim != c.ref_all.prim).mean() > 0.05
    _check(c, g)


def test_shapes_closest_and_occlusion():
    c = case("shapes")
    g = Renderer(c.cfg)
    assert g.octree()["depth"] >= 2 and len(c.cfg.model.shapes) == 7
    _check(c, g)
