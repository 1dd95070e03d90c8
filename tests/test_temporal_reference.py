"""CPU: the temporal stage's numpy restatement (tests/temporal_reference.py) on its own — the
properties k_temporal_accumulate inherits by matching it bit for bit (tests/test_gpu_temporal.py) — and
scene.world_to_film against the oracle's own rays."""
import dataclasses
import math

import numpy as np
import pytest

import denoise_reference as dref
import temporal_reference as ref
from computational_ray_tracer_amd import capi, scene
from computational_ray_tracer_amd.renderer import records_to_arrays

F32 = np.float32
bits = ref.bits


# ------------------------------------------------------------------------------------ world_to_film
def cornell_view(camera, res):
    """The Cornell box through `camera` under the reference integrator without culling (the oracle's sample records
    then hold every camera ray and its first hit), box filter of the pixel's footprint, 2 x 2 jittered strata."""
    return scene.Config("cornell_view", dataclasses.replace(scene.cornell_box(), cull_backfaces=False), camera,
                        scene.StratifiedSampler(2, 2, True, 0), scene.Film(res=res, filter=capi.RT_FILTER_BOX),
                        scene.Integrator(capi.RT_INTEGRATOR_REFERENCE), 0, 4)


def turned(cls, res, **kw):
    """A camera moved off the box's axis and turned (yaw and a little pitch)."""
    yaw, pitch = math.radians(9.0), math.radians(-4.0)
    look = (math.sin(yaw) * math.cos(pitch), math.sin(pitch), math.cos(yaw) * math.cos(pitch))
    return cls(position=(240.0, 300.0, -780.0), look=look, right=(1, 0, 0), worldup=(0, 1, 0), res=res, **kw)


VIEWS = {
    "perspective48": lambda: turned(scene.PerspectiveCamera, (48, 48), near=1.0, far=5000.0, fov=62.0, aspect_fix=True),
    "orthographic48": lambda: turned(scene.OrthographicCamera, (48, 48), near=1e-2, far=5000.0, sensor=(700.0, 700.0)),
    "perspective64x40": lambda: turned(scene.PerspectiveCamera, (64, 40), near=1.0, far=5000.0, fov=62.0,
                                       aspect_fix=True),
}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_world_to_film_lands_every_oracle_hit_in_its_own_pixel(oracle_lib, view):
    """Every hit point ro + t rd of the oracle's sample records, pushed through the matrix in float64, lands within
    0.5 + 1e-3 of its own pixel's centre in both axes; a pixel's frustum is convex, so the mean of its hit points
    (what the stage projects) lands there too."""
    cam = VIEWS[view]()
    W, H = cam.res
    o = oracle_lib.OracleScene(cornell_view(cam, (W, H)))
    M = scene.world_to_film(cam)
    assert M.dtype == np.float32 and M.shape == (16,)
    M = M.astype(np.float64).reshape(4, 4).T           # row-major float64
    px = np.arange(W * H, dtype=np.int32)
    cx, cy = px % W + 0.5, px // W + 0.5
    psum, cnt = np.zeros((W * H, 3)), np.zeros(W * H)

    def check(P, sel, what):
        q = np.concatenate([P, np.ones((len(P), 1))], axis=1) @ M.T
        assert np.all(q[:, 3] > 0), what
        u, v = q[:, 0] / q[:, 3], q[:, 1] / q[:, 3]
        du, dv = np.abs(u - cx[sel]).max(), np.abs(v - cy[sel]).max()
        print(f"{view} {what}: max |du| {du:.6f} max |dv| {dv:.6f} over {len(P)} points")
        assert du <= 0.5 + 1e-3 and dv <= 0.5 + 1e-3, what

    for i in range(4):
        r = records_to_arrays(o.samples(px, np.full(W * H, i, np.int32)))
        hit = r["prim"] >= 0
        assert hit.sum() > W * H // 4
        P = r["ro"][hit].astype(np.float64) + r["t"][hit].astype(np.float64)[:, None] * r["rd"][hit].astype(np.float64)
        check(P, hit, f"index {i}")
        psum[hit] += P
        cnt[hit] += 1
    some = cnt > 0
    check(psum[some] / cnt[some][:, None], some, "pixel means")


def test_world_to_film_rejects_other_cameras():
    with pytest.raises(TypeError):
        scene.world_to_film(scene.PinholeCamera())
    with pytest.raises(TypeError):
        scene.world_to_film(scene.ThinlensCamera())


# ------------------------------------------------------------------------------------ synthetic properties
def pick_xy(shift=(0.0, 0.0), w=1.0):
    """M with X = P.x + shift_x, Y = P.y + shift_y, Wc = w (column-major)."""
    M = np.zeros(16, F32)
    M[0], M[5], M[12], M[13], M[15] = 1, 1, shift[0], shift[1], w
    return M


def flat_frame(W, H, rng, n, k=4, z=F32(300.0), normal=(0.0, 0.0, 1.0), colour=None):
    """A frame whose first hits sit at the pixel centres of the plane z, facing `normal`: (film, mom, feat, pos)."""
    N = W * H
    y, x = np.divmod(np.arange(N), W)
    c = rng.uniform(0.1, 2.0, (N, 3)).astype(F32) if colour is None else np.broadcast_to(F32(colour), (N, 3))
    nn = np.full(N, n, F32)
    film = np.concatenate([c * nn[:, None], nn[:, None]], axis=1).astype(F32)
    s = rng.uniform(0.5, 4.0, N).astype(F32)
    mom = np.stack([s * nn, (s * s + F32(0.3)) * nn], axis=1).astype(F32)
    feat = np.concatenate([np.broadcast_to(F32(normal) * F32(k), (N, 3)), np.full((N, 1), F32(k) * F32(500.0))],
                          axis=1).astype(F32)
    pos = np.stack([x + F32(0.5), y + F32(0.5), np.full(N, z, F32), np.ones(N, F32)], axis=1).astype(F32)
    return film, mom, feat, pos


P = dict(ref.DEFAULTS)


def test_pixel_exact_reprojection_is_the_exact_mean():
    W, H = 13, 9
    rng = np.random.default_rng(3)
    cur, hist = flat_frame(W, H, rng, 8), flat_frame(W, H, rng, 8)
    of, om, cnt = ref.accumulate(*cur, hist, pick_xy(), W, H, **P)
    assert cnt == dict(reprojected=W * H, disoccluded=0, background=0)
    assert np.all(of[:, 3] == 16)
    mean = ((cur[0][:, :3] / F32(8) + hist[0][:, :3] / F32(8)) * F32(0.5)).astype(F32)     # alpha = 1/2 is exact
    assert np.array_equal(bits(of[:, :3]), bits(mean * F32(16)))
    m = ((cur[1] / F32(8) + hist[1] / F32(8)) * F32(0.5)).astype(F32)
    assert np.array_equal(bits(om), bits(m * F32(16)))
    # a constant colour comes out bit-equal
    col = (0.3, 0.7, 1.1)
    cur, hist = flat_frame(W, H, rng, 8, colour=col), flat_frame(W, H, rng, 8, colour=col)
    of, _, _ = ref.accumulate(*cur, hist, pick_xy(), W, H, **P)
    assert np.array_equal(bits(of[:, :3] / of[:, 3:4]), bits(cur[0][:, :3] / cur[0][:, 3:4]))


@pytest.mark.parametrize("shift", [(3, 0), (-2, 0), (0, 2), (-1, -3)])
def test_integer_shift_fetches_the_shifted_pixel(shift):
    W, H = 13, 9
    rng = np.random.default_rng(5)
    cur, hist = flat_frame(W, H, rng, 4), flat_frame(W, H, rng, 12)
    of, om, cnt = ref.accumulate(*cur, hist, pick_xy(shift), W, H, **P)
    y, x = np.divmod(np.arange(W * H), W)
    xs, ys = x + shift[0], y + shift[1]
    inside = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    src = np.where(inside, ys * W + xs, 0)
    assert cnt == dict(reprojected=int(inside.sum()), disoccluded=int((~inside).sum()), background=0)
    # off the image: the current frame, bit for bit
    assert np.array_equal(bits(of[~inside]), bits(cur[0][~inside]))
    assert np.array_equal(bits(om[~inside]), bits(cur[1][~inside]))
    # inside: n' = 16, alpha = 1/4, the history is exactly the shifted pixel's mean
    al = F32(0.25)
    ch = (hist[0][src, :3] / F32(12)).astype(F32)
    c2 = ((F32(1) - al) * ch + al * (cur[0][:, :3] / F32(4))).astype(F32)
    assert np.all(of[inside, 3] == 16)
    assert np.array_equal(bits(of[inside, :3]), bits((c2 * F32(16))[inside]))


def test_rejections_give_the_current_frame_bit_for_bit():
    W, H = 13, 9
    rng = np.random.default_rng(9)
    cur = flat_frame(W, H, rng, 4)
    lim = float(F32(P["plane_rel"]) * F32(500.0))                     # plane_rel * z_p
    cases = {
        "plane moved along the normal": (flat_frame(W, H, rng, 4, z=F32(300.0) + F32(lim * 1.01)), pick_xy()),
        "turned normal": (flat_frame(W, H, rng, 4, normal=(1.0, 0.0, 0.0)), pick_xy()),
        "Wc == 0": (flat_frame(W, H, rng, 4), pick_xy(w=0.0)),
        "Wc < 0": (flat_frame(W, H, rng, 4), pick_xy(w=-1.0)),
        "NaN matrix": (flat_frame(W, H, rng, 4), pick_xy(shift=(np.nan, 0.0))),
    }
    for name, (hist, M) in cases.items():
        of, om, cnt = ref.accumulate(*cur, hist, M, W, H, **P)
        assert cnt == dict(reprojected=0, disoccluded=W * H, background=0), name
        assert np.array_equal(bits(of), bits(cur[0])) and np.array_equal(bits(om), bits(cur[1])), name
    # just inside the plane tolerance the history is taken
    hist = flat_frame(W, H, rng, 4, z=F32(300.0) + F32(lim * 0.99))
    assert ref.accumulate(*cur, hist, pick_xy(), W, H, **P)[2]["reprojected"] == W * H
    # no history at all: the inputs; pixels without samples come out zero, pixels without hits are background
    film, mom, feat, pos = (a.copy() for a in cur)
    film[:3], mom[:3] = 0, 0
    pos[5:9] = 0
    of, om, cnt = ref.accumulate(film, mom, feat, pos, None, None, W, H, **P)
    assert np.array_equal(bits(of), bits(film)) and np.array_equal(bits(om), bits(mom))
    assert cnt == dict(reprojected=0, disoccluded=W * H - 7, background=4)


def test_history_length_is_capped():
    """n' never exceeds max_history, unless n alone does; fractional taps, random counts."""
    W, H = 17, 11
    rng = np.random.default_rng(11)
    cur, hist = flat_frame(W, H, rng, 4), flat_frame(W, H, rng, 4)
    n_cur = rng.integers(1, 40, W * H).astype(F32)
    n_hist = rng.integers(1, 40, W * H).astype(F32)
    for fr, nn in ((cur, n_cur), (hist, n_hist)):
        fr[0][:] = np.concatenate([fr[0][:, :3] / F32(4) * nn[:, None], nn[:, None]], axis=1)
    of, _, cnt = ref.accumulate(*cur, hist, pick_xy((0.37, 0.61)), W, H, **dict(P, max_history=24.0))
    assert cnt["reprojected"] > W * H // 2
    n2 = of[:, 3]
    assert np.all(n2 <= np.maximum(F32(24.0), n_cur)) and np.all(n2 >= n_cur)
    assert np.any(n2 == 24) and np.any(n_cur > 24)


# ------------------------------------------------------------------------------------ quality on the oracle
FRAMES, SPP_SIDE = 6, 2


def moving_wide_cornell(f, res, side, seed):
    """Frame f of the camera path (translation plus yaw) over the wide Cornell view of tests/test_denoise_reference.py
    (fov 100: the frame's border looks past the box)."""
    yaw = math.radians(1.5 * f)
    cam = scene.PerspectiveCamera(near=1.0, far=5000.0, fov=100.0, position=(278.0 - 12.0 * f, 273.0 + 4.0 * f,
                                                                             -800.0 + 10.0 * f),
                                  look=(math.sin(yaw), 0.0, math.cos(yaw)), right=(1, 0, 0), worldup=(0, 1, 0), res=res,
                                  lens_radius=0.0, focal_distance=0.0, aspect_fix=True)
    return scene.Config("cornell_wide_moving", scene.cornell_box(), cam, scene.StratifiedSampler(side, side, True, seed),
                        scene.Film(res=res, filter=capi.RT_FILTER_BOX),
                        scene.Integrator(capi.RT_INTEGRATOR_PATH, max_depth=5), 0, side * side)


def oracle_frame(oracle_lib, cfg, W, H, k):
    """(film, mom, feat, pos) of cfg's samples, everything from the oracle."""
    o = oracle_lib.OracleScene(cfg)
    film, mom = np.zeros((W * H, 4), F32), np.zeros((W * H, 2), F32)
    for i in range(cfg.index_end):
        c = o.render(i, i + 1)
        film = film + c
        v = (c[:, 0] + c[:, 1]) + c[:, 2]
        mom[:, 0] = mom[:, 0] + v
        mom[:, 1] = mom[:, 1] + v * v
    rc = dref.record_config(cfg)
    orc = oracle_lib.OracleScene(rc)
    feat = dref.oracle_features(orc, dref.world_triangles(rc.model), W, H, 0, k)
    pos = ref.oracle_positions(orc, W, H, 0, k)
    return film, mom, feat, pos


def test_quality_on_a_moving_oracle_camera(oracle_lib):
    """48 x 48 wide Cornell view, 4 spp per frame, 6 frames of a moving camera, every input from the oracle: on the
    last frame MSE(accumulated + filtered) < MSE(filtered only) < MSE(raw) against the oracle's 256-spp film of that
    view, at TEMPORAL_DEFAULTS and DENOISE_DEFAULTS.

    Measured when the defaults were frozen (MSE of the mean colour over all pixels and channels): raw 1.360e-04,
    filtered only 1.291e-04, accumulated only 9.065e-05, accumulated + filtered 9.626e-05; 103 pixels reprojected, 66
    disoccluded, 2135 background on the last frame (the box covers about 13 x 13 pixels, most of which straddle two
    surfaces).  DESIGN.md §3d has the sweep over three views."""
    W = H = 48
    k = P["feature_samples"]
    hist, M_prev, last = None, None, None
    for f in range(FRAMES):
        cfg = moving_wide_cornell(f, (W, H), SPP_SIDE, seed=f)
        film, mom, feat, pos = oracle_frame(oracle_lib, cfg, W, H, k)
        acc_f, acc_m, cnt = ref.accumulate(film, mom, feat, pos, hist, M_prev, W, H, **P)
        print(f"frame {f}: {cnt}")
        assert sum(cnt.values()) == W * H
        hist, M_prev, last = (acc_f, acc_m, feat, pos), scene.world_to_film(cfg.camera), (film, mom, feat)
    assert cnt["reprojected"] > 0 and cnt["background"] > 0       # (the box covers about 13 x 13 pixels of this view)
    truth = oracle_lib.OracleScene(moving_wide_cornell(FRAMES - 1, (W, H), 16, seed=0)).render(0, 256)
    truth = truth[:, :3].astype(np.float64) / truth[:, 3:4]

    def mse(f):
        return float(np.mean((f[:, :3].astype(np.float64) / f[:, 3:4] - truth) ** 2))
    film, mom, feat = last
    raw = mse(film)
    filt = mse(dref.denoise(film, mom, feat, W, H, **dref.DEFAULTS)[0])
    acc = mse(hist[0])
    both = mse(dref.denoise(hist[0], hist[1], feat, W, H, **dref.DEFAULTS)[0])
    print(f"MSE against 256 spp: raw {raw:.4e}, filtered {filt:.4e}, accumulated {acc:.4e}, "
          f"accumulated + filtered {both:.4e}")
    assert both < filt < raw
