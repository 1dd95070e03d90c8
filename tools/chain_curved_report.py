#!/usr/bin/env python3
"""Curved specular-chain guides on the mixed scene (CFG4: a mirror sphere and a BK7 glass sphere) along the camera path
of tools/chain_report.py: chain_depth 0, 4 and 4 | RT_CHAIN_CURVED side by side -> a JSON file.

usage: tools/chain_curved_report.py [--res 1920x1080] [--frames 6] [--spp-side 2] [--truth-side 16] [--frequency 70]
                                    [--repeat 7] [--out profiles/chain_curved_cfg4.json]

Needs an MI355X.  Every frame renders spp-side^2 uniform samples per pixel (the sampler's seed is the frame number) in
three temporal sessions with the filter: first-surface guides, planar chain guides and curved chain guides.  Per frame
and session it reports the pixel classes of rt_temporal_frame, the mean accumulated sample count n' and the MSE of the
mean colour against a uniform truth-side^2 film of that frame's view over three sets of pixels: those whose guides
change between depth 0 and the planar depth 4, those among them whose curved guides differ from the planar ones, and
the rest.  The guide pass alone (rt_render_features_chain, host films, the blocking call) is timed for the three modes
in turn, --repeat rounds, best and median."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CHAIN = 4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--frames", type=int, default=6)
    p.add_argument("--spp-side", type=int, default=2)
    p.add_argument("--truth-side", type=int, default=16)
    p.add_argument("--frequency", type=int, default=70)
    p.add_argument("--repeat", type=int, default=7)
    p.add_argument("--out", default=str(ROOT / "profiles" / "chain_curved_cfg4.json"))
    a = p.parse_args()
    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import DENOISE_DEFAULTS, TEMPORAL_DEFAULTS, Renderer

    W, H = (int(v) for v in a.res.split("x"))
    spp, truth_spp = a.spp_side ** 2, a.truth_side ** 2
    k = TEMPORAL_DEFAULTS["feature_samples"]
    dev = torch.cuda.current_device()
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    modes = {"depth0": dict(chain_depth=0), "planar": dict(chain_depth=CHAIN),
             "curved": dict(chain_depth=CHAIN, chain_curved=True)}

    def camera(f):
        """Frame f of the path of tools/chain_report.py: translation plus yaw through the Cornell view."""
        yaw = math.radians(1.0 * f)
        return scene.PerspectiveCamera(near=1.0, far=5000.0, fov=62.0,
                                       position=(278.0 + 8.0 * f, 273.0 - 3.0 * f, -800.0 + 6.0 * f),
                                       look=(math.sin(yaw), 0.0, math.cos(yaw)), right=(1, 0, 0), worldup=(0, 1, 0),
                                       res=(W, H), lens_radius=0.0, focal_distance=0.0, aspect_fix=True)

    def set_frame(r, f, side):
        r.set_camera(camera(f))
        r._chk("rt_sampler_set", r.lib.rt_sampler_set(r.h, C.byref(scene.StratifiedSampler(side, side, True, f).desc())))

    cfg = scene.cfg4_mixed(res=(W, H), spp=(a.spp_side, a.spp_side), frequency=a.frequency)
    r_truth = Renderer(scene.cfg4_mixed(res=(W, H), spp=(a.truth_side, a.truth_side), frequency=a.frequency), device=dev)
    r_plain = Renderer(cfg, device=dev)
    sessions = {m: Renderer(cfg, device=dev) for m in modes}
    for m, r in sessions.items():
        r.temporal_begin(**modes[m])
    film_t = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    out = {"config": cfg.name, "res": [W, H], "frame_spp": spp, "truth_spp": truth_spp, "chain_depth": CHAIN,
           "temporal": dict(TEMPORAL_DEFAULTS), "denoise": dict(DENOISE_DEFAULTS), "library": capi.library_sha16(),
           "frames": []}
    for f in range(a.frames):
        film_t.zero_()
        set_frame(r_truth, f, a.truth_side)
        r_truth.render_pass_device(0, truth_spp, film_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        truth = film_t.cpu().numpy().astype(np.float64)
        truth = truth[:, :3] / truth[:, 3:4]
        M = scene.world_to_film(camera(f))
        for r in (r_plain, *sessions.values()):
            set_frame(r, f, a.spp_side)
        raw, _, _ = r_plain.render_adaptive(spp, spp, spp, 0.0)
        films, infos = {}, {}
        for m, r in sessions.items():
            films[m], infos[m] = r.temporal_frame(M, spp, denoise=dict(modes[m]))
        # the guide pass alone, the three modes in turn
        ts, guides, rays = {m: [] for m in modes}, {}, {}
        for _ in range(a.repeat):
            for m, kw in modes.items():
                r_plain.reset_stats()
                t0 = time.perf_counter()
                guides[m] = r_plain.render_features_chain(0, k, kw["chain_depth"], chain_curved=kw.get("chain_curved", False))
                ts[m].append((time.perf_counter() - t0) * 1e3)
                rays[m] = r_plain.stats()["rays"]
        differ = lambda x, y: np.any(bits(guides[x][0]) != bits(guides[y][0]), axis=1) | \
            np.any(bits(guides[x][1]) != bits(guides[y][1]), axis=1)
        changed = differ("depth0", "planar")
        moved = differ("planar", "curved")

        def mse(x, sel):
            if not sel.any():
                return None
            return float(np.mean((x[sel, :3].astype(np.float64) / np.maximum(x[sel, 3:4], 1) - truth[sel]) ** 2))
        row = {"frame": f, "pixels_changed": int(changed.sum()), "pixels_curved_moved": int(moved.sum()),
               "pixels_rest": int((~changed).sum()), "camera_rays": rays["depth0"],
               "continuation_rays": rays["planar"] - rays["depth0"],
               "continuation_rays_curved": rays["curved"] - rays["depth0"]}
        for m in modes:
            row[m] = {"classes": {c: infos[m][c] for c in ("reprojected", "disoccluded", "background")},
                      "mean_n": float(np.mean(films[m][:, 3].astype(np.float64))),
                      "mean_n_changed": float(np.mean(films[m][changed, 3].astype(np.float64))) if changed.any() else None,
                      "guide_pass_ms_best": round(min(ts[m]), 3),
                      "guide_pass_ms_median": round(statistics.median(ts[m]), 3),
                      "mse_changed": mse(films[m], changed), "mse_curved_moved": mse(films[m], moved),
                      "mse_rest": mse(films[m], ~changed)}
        row["raw"] = {"mse_changed": mse(raw, changed), "mse_curved_moved": mse(raw, moved), "mse_rest": mse(raw, ~changed)}
        out["frames"].append(row)
        print(json.dumps(row), flush=True)
    for r in sessions.values():
        r.temporal_end()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
