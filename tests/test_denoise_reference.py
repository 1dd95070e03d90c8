"""CPU: the denoiser's numpy restatement (tests/denoise_reference.py) on its own — the properties the
GPU kernels inherit by matching it bit for bit (tests/test_gpu_denoise.py)."""
import numpy as np
import pytest

import denoise_reference as ref
from computational_ray_tracer_amd import capi, scene

F32 = np.float32
bits = ref.bits


@pytest.mark.parametrize("npl", [0, 7])
@pytest.mark.parametrize("res", [(24, 17), (70, 50)])
def test_exact_edge_preservation(res, npl):
    """Two regions with orthogonal normals, colour 0 on one side and 1 on the other, noisy moments: the cross-region
    normal weight is max(0, 0) = 0 exactly, and inside a region sum(w * 1) and sum(w) are the same float sums, so the
    output equals the input bit for bit on both sides, at every iteration count."""
    W, H = res
    rng = np.random.default_rng(7)
    y, x = np.divmod(np.arange(W * H), W)
    right = x * 3 + y >= (W * 3 + H) // 2            # a slanted edge
    k, n = 4, F32(16)
    feat = np.zeros((W * H, 4), F32)
    feat[~right, 0] = k
    feat[right, 1] = k
    feat[:, 3] = k * F32(500)
    film = np.zeros((W * H, 4), F32)
    film[right, :3] = n
    film[:, 3] = n
    s = film[:, :3].sum(axis=1)
    noise = rng.uniform(0.0, 30.0, W * H).astype(F32)  # sumsq >= sum^2 / n: any non-negative variance
    mom = np.stack([s, s * s / n + noise], axis=1).astype(F32)
    for it in (1, 5, 6):
        out, var = ref.denoise(film, mom, feat, W, H, **dict(ref.DEFAULTS, iterations=it, normal_power_log2=npl))
        assert np.array_equal(bits(out), bits(film))
        assert np.all(var >= 0) and var.max() > 0


def wide_cornell(res, side):
    """The wide Cornell view of tests/test_gpu_adaptive.py (fov 100: the frame's border looks past the box), with
    side^2 stratified samples per pixel."""
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=100.0, position=(278.0, 273.0, -800.0), look=(0, 0, 1),
                                  right=(1, 0, 0), worldup=(0, 1, 0), res=res, lens_radius=0.0, focal_distance=0.0,
                                  aspect_fix=True)
    return scene.Config("cornell_wide", scene.cornell_box(), cam, scene.StratifiedSampler(side, side, True, 0),
                        scene.Film(res=res, filter=capi.RT_FILTER_BOX),
                        scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=5), 0, side * side)


def test_usefulness_on_an_oracle_render(oracle_lib):
    """Cornell 64x64 wide view, 16 spp, every input from the oracle: the reference filter at the default parameters
    gives a strictly lower MSE against the oracle's 256-spp film than the unfiltered 16-spp film.

    Measured when the defaults were frozen (MSE of the mean colour over all pixels and channels): unfiltered
    2.670e-05; defaults (sigma_l 1.5, lum_floor 0.01, depth_floor 0.002) 2.568e-05.  In this view the box covers only
    16x16 pixels, so shading changes within a few pixels: with sigma_l 4 the same filter gives 4.901e-05 here (worse
    than unfiltered), which is why the default is 1.5 (DESIGN.md §3c has the sweep over three views)."""
    W = H = 64
    cfg = wide_cornell((W, H), 4)
    o = oracle_lib.OracleScene(cfg)
    film, mom = np.zeros((W * H, 4), F32), np.zeros((W * H, 2), F32)
    for i in range(16):
        c = o.render(i, i + 1)
        film = film + c
        v = (c[:, 0] + c[:, 1]) + c[:, 2]
        mom[:, 0] = mom[:, 0] + v
        mom[:, 1] = mom[:, 1] + v * v
    assert np.array_equal(bits(film), bits(o.render(0, 16)))
    rc = ref.record_config(cfg)   # the reference integrator with culling off: the same rays and first hits
    feat = ref.oracle_features(oracle_lib.OracleScene(rc), ref.world_triangles(rc.model), W, H, 0, 4)
    assert 0 < np.count_nonzero(feat[:, 3]) < W * H       # the view has camera misses
    truth = oracle_lib.OracleScene(wide_cornell((W, H), 16)).render(0, 256)
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]

    def mse(f):
        return float(np.mean((f[:, :3].astype(np.float64) / f[:, 3:4] - truth) ** 2))
    out, _ = ref.denoise(film, mom, feat, W, H, **ref.DEFAULTS)
    assert np.array_equal(bits(out[:, 3]), bits(film[:, 3]))
    before, after = mse(film), mse(out)
    print(f"MSE against 256 spp: unfiltered {before:.4e}, filtered {after:.4e}")
    assert after < before
