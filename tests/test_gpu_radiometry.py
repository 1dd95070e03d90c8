"""GPU: the path kernels against closed-form radiometry (tests/radiometry_reference.py, numpy float64).

For every case and variant: (1) the GPU film is the oracle's bit for bit, the project's standard check; (2) the GPU
film itself passes the closed-form comparison, so the physics stays pinned even if (1) were ever relaxed; (3) the
kernels that ran are the intended ones (rt_stats, rt_octree_info).  The environment knobs are left alone: the parity
tests cover them bit for bit.

The colour cases (ref.COLOUR_CASES) run through the same test.  Within a scene they change the film's sensor while the
renderer is kept (ref.scene_key), so a sensor curve left over from the previous variant would fail (2);
tests/test_gpu_spectral.py checks that transition on its own."""
import ctypes as C

import numpy as np
import pytest

import radiometry_reference as ref
from computational_ray_tracer_amd import capi
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Shared:
    """One Renderer per scene, reused by that scene's depth and integrator variants (ref.scene_key; the variants are
    adjacent in ref.CASES), released when the next scene arrives."""
    key = None
    renderer = None


@pytest.fixture(scope="module")
def shared():
    s = _Shared()
    yield s
    if s.renderer is not None:
        s.renderer.close()


def _renderer(shared, case_id, cfg):
    key = ref.scene_key(case_id)
    if shared.key != key:
        if shared.renderer is not None:
            shared.renderer.close()
        shared.renderer, shared.key = Renderer(), key
    shared.renderer.configure(cfg)
    return shared.renderer


def _octree_info(g):
    info = capi.rt_octree_info()
    g._chk("rt_octree_get_info", g.lib.rt_octree_get_info(g.h, C.byref(info)))
    return info


@pytest.mark.parametrize("case_id", ref.CASE_IDS)
def test_gpu_film_is_the_oracle_s_and_matches_the_closed_form(shared, oracle_lib, case_id):
    cfg, mu, vmax, include, spp = ref.build_case(case_id)
    assert cfg.film.res[0] * cfg.film.res[1] * spp <= 64 * 64 * 256
    g = _renderer(shared, case_id, cfg)
    g.reset_stats()
    fg = g.render_pass(0, spp)
    st = g.stats()

    # (1) bit-identical to the oracle's film of the same Config
    fo = oracle_lib.OracleScene(cfg).render(0, spp)
    bad = np.any(bits(fg) != bits(fo), axis=1)
    assert bad.sum() == 0, f"{bad.sum()} pixels differ; max |diff| {np.abs(fg - fo).max()}"

    # (2) the closed form, directly
    rows = ref.compare(fg, mu, vmax, include, spp)
    print(f"{case_id}: max |got - mu| / tol = {ref.deviation(rows):.3f}\n{ref.report(rows)}")
    assert ref.passes(rows), ref.report(rows)
    for factor in (1.03, 0.97):                      # and it would not pass with a 3 % error
        assert not ref.passes(ref.compare(fg, factor * mu, vmax, include, spp))

    # (3) the path taken
    assert st["samples"] == cfg.film.res[0] * cfg.film.res[1] * spp
    assert st["coop_overflows"] == 0
    info = _octree_info(g)
    if "tess" in case_id:
        assert info.depth > 0 and info.bvh_nodes > 0, "the tessellated floor must build a multi-level octree"
    else:
        assert info.depth == 0
    if case_id.startswith("k3_quad") and "_path_" in case_id:
        assert st["nee_vertices"] == 0, "PATH with one quad light and no shapes runs k_path_shade / k_path_shadow"
        assert st["shadow_rays"] > 0
    elif case_id.startswith(("k1", "k2", "k3", "k4", "k5")):
        assert st["nee_vertices"] > 0, "k_path_shade_full + k_path_nee"
    elif case_id.startswith("kref"):
        assert st["nee_vertices"] == 0 and st["shadow_rays"] == 0, "the reference Li traces camera rays only"
