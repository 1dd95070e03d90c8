"""CPU: the guided estimate's numpy restatement (tests/guided_reference.py) on its own, and a guided
against an unguided session replayed on the oracle's moving-camera frames.  Nothing here uses the GPU."""
import dataclasses

import numpy as np

import denoise_reference as dref
import guided_reference as gref
import temporal_reference as tref
from computational_ray_tracer_amd import scene
from test_gpu_adaptive import ref_block_error
from test_gpu_temporal import synthetic
from test_temporal_reference import flat_frame, moving_wide_cornell, pick_xy

F32 = np.float32
bits = tref.bits
P = dict(tref.DEFAULTS)


def test_no_history_is_the_plain_estimate():
    """Without a history the guided block error is k_adaptive_error's of the film itself, bit for bit; and the
    module's block_error is the one tests/test_gpu_adaptive.py holds k_adaptive_error to."""
    for W, H in ((1, 1), (8, 8), (37, 29), (131, 67)):
        cur, _, _ = synthetic(W, H, seed=W)
        plain = gref.block_error(cur[0], cur[1], W, H, 1e-3)
        assert plain.shape == ((H + 7) // 8, (W + 7) // 8)
        assert np.array_equal(bits(gref.guided_block_error(*cur, None, None, W, H, 1e-3, **P)), bits(plain))
        assert np.array_equal(bits(plain), bits(ref_block_error(cur[0], cur[1], W, H, 1e-3)))


def test_pooling_equal_moments_only_shrinks_the_error():
    """A static orthographic view whose taps fall on the pixel centres (a = b = 0), the history's per-sample moments
    equal to the current ones with nh = 3 n.  Pooling samples of equal moments leaves the mean and the population
    variance v as they are, and sem = sqrt(((n v) / (n - 1)) / n) = sqrt(v / (n - 1)), so sem' = sem sqrt((n - 1) /
    (n' - 1)) <= sem: every block's guided error is at most its plain error (the 1e-5 covers the float32 rounding of
    the blend, of relative size 2^-23 per operation), and smaller by that factor."""
    W, H = 29, 19
    rng = np.random.default_rng(17)
    n = 4
    cur = flat_frame(W, H, rng, n)
    hist = (cur[0] * F32(3), cur[1] * F32(3), cur[2], cur[3])
    plain = gref.block_error(cur[0], cur[1], W, H, 1e-3)
    acc_f, _, cnt = tref.accumulate(*cur, hist, pick_xy(), W, H, **P)
    assert cnt["reprojected"] == W * H and np.all(acc_f[:, 3] == 4 * n)
    guided = gref.guided_block_error(*cur, hist, pick_xy(), W, H, 1e-3, **P)
    assert np.all(plain > 0)
    assert np.all(guided <= plain * F32(1 + 1e-5))
    ratio = guided.astype(np.float64) / plain
    assert np.allclose(ratio, np.sqrt((n - 1) / (4 * n - 1)), rtol=1e-4)


# ------------------------------------------------------------------------------------ sessions on the oracle
FRAMES, SIDE = 6, 4
SESSION = dict(min_samples=4, step_samples=4, max_samples=16, rel_error=0.1, abs_floor=1e-3)


def oracle_levels(oracle_lib, cfg, W, H, stops):
    """levels[k] = (film, mom) of the first k indices, per-index OracleScene.render."""
    o = oracle_lib.OracleScene(cfg)
    film, mom, levels = np.zeros((W * H, 4), F32), np.zeros((W * H, 2), F32), {}
    for i in range(max(stops)):
        c = o.render(i, i + 1)
        film = film + c
        v = (c[:, 0] + c[:, 1]) + c[:, 2]
        mom = np.stack([mom[:, 0] + v, mom[:, 1] + v * v], axis=1)
        if i + 1 in stops:
            levels[i + 1] = (film.copy(), mom.copy())
    return levels


def run_path(oracle_lib, res, fov=100.0, truth=True):
    """The six-frame path with 16 strata per frame and the SESSION descriptor: an unguided session (the plain
    estimate, then the stage) against a guided one (simulate_frame), each with its own history, every input from the
    oracle.  Per frame: {samples_unguided, samples_guided, mse_unguided, mse_guided (accumulated + filtered against the
    oracle's 256-spp film of the view, with truth), reprojected}."""
    W, H = res
    k = P["feature_samples"]
    hist = {"unguided": None, "guided": None}
    M_prev, rows = None, []

    def config(f, side, seed):
        cfg = moving_wide_cornell(f, res, side, seed)
        return dataclasses.replace(cfg, camera=dataclasses.replace(cfg.camera, fov=fov))
    for f in range(FRAMES):
        cfg = config(f, SIDE, f)
        levels = oracle_levels(oracle_lib, cfg, W, H, (4, 8, 12, 16))
        rc = dref.record_config(cfg)
        orc = oracle_lib.OracleScene(rc)
        feat = dref.oracle_features(orc, dref.world_triangles(rc.model), W, H, 0, k)
        pos = tref.oracle_positions(orc, W, H, 0, k)
        if truth:
            t = oracle_lib.OracleScene(config(f, 16, 0)).render(0, 256)
            t = t[:, :3].astype(np.float64) / t[:, 3:4]
        row = {}
        for which in ("unguided", "guided"):
            h = hist[which]
            sim = gref.simulate_frame(levels, feat, pos, h if which == "guided" else None, M_prev, W, H, **SESSION, **P)
            film, mom, samples = sim["film"], sim["mom"], sim["samples"]
            assert samples == int(film[:, 3].sum()) and sim["index_done"] <= 16
            assert np.all((film[:, 3] >= 4) & (film[:, 3] <= 16))
            acc_f, acc_m, cnt = tref.accumulate(film, mom, feat, pos, h, M_prev, W, H, **P)
            hist[which] = (acc_f, acc_m, feat, pos)
            row["samples_" + which] = samples
            if truth:
                out = dref.denoise(acc_f, acc_m, feat, W, H, **dref.DEFAULTS)[0]
                row["mse_" + which] = float(np.mean((out[:, :3].astype(np.float64) / out[:, 3:4] - t) ** 2))
        row["reprojected"] = cnt["reprojected"]
        rows.append(row)
        M_prev = scene.world_to_film(cfg.camera)
        print(f"{W}x{H} fov {fov:g} frame {f}: {row}")
    return rows


def test_guided_against_unguided_on_a_moving_oracle_camera(oracle_lib):
    """The first row of DESIGN.md §3f's CPU table: the 48 x 48, fov 100 path of tests/test_temporal_reference.py.

    Measured: both sessions render 12288 samples in every one of the six frames (2304 pixels x 4, then 12 blocks x 64
    pixels x 4 more) and so produce the same films, MSE 9.0205e-05 on the last frame.  The ordering is therefore not
    "fewer samples in the last frame" but "as many": the box covers 13 x 13 pixels of this view, 83 to 103 of them
    reproject and about 70 are disoccluded, so every 8x8 block that is open after the first iteration holds pixels
    without history, and the block is the unit.  That is what is asserted, with "never more" for every frame.  The
    other two views of §3d's table (run_path(oracle_lib, (96, 96)) and (..., fov=40.0), 13 s and 44 s, not run here)
    do differ: 45824 against 49152 samples on the last frame at fov 100, 96000 against 140800 at fov 40, at a higher
    MSE (DESIGN.md §3f has the table)."""
    rows = run_path(oracle_lib, (48, 48))
    assert rows[0]["samples_guided"] == rows[0]["samples_unguided"]                 # no history: the plain estimate
    assert all(r["samples_guided"] <= r["samples_unguided"] for r in rows)
    assert rows[-1]["samples_guided"] == rows[-1]["samples_unguided"] == 12288
    assert rows[-1]["reprojected"] > 0
