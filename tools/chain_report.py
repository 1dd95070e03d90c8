#!/usr/bin/env python3
"""Specular-chain guides on the mixed scene (CFG4: a mirror sphere and a BK7 glass sphere) along a camera path: error
with chain_depth 0 against chain_depth 4, pixel classes and the time of the guide pass -> one JSON line.

usage: tools/chain_report.py [--res 1920x1080] [--frames 6] [--spp-side 2] [--truth-side 16] [--frequency 70]
                             [--repeat 5] [--out report.json]

Needs an MI355X.  The camera translates and yaws from frame to frame; every frame renders spp-side^2 uniform samples
per pixel (the sampler's seed is the frame number) in two temporal sessions with the filter, one with first-surface
guides (chain_depth 0) and one with chain guides (chain_depth 4).  Per frame it reports, for both, the pixel classes of
rt_temporal_frame and the MSE of the mean colour against a uniform truth-side^2 film of that frame's view, separately
over the pixels whose guides change (their feature or position film differs in bits between the two depths) and over
the rest, next to the MSE of the raw frame; and the wall time (best of --repeat, the blocking call, host films) of
rt_render_features_chain at depth 0 and at depth 4 with the continuation rays it traced."""
import argparse
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

CHAIN = 4


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--frames", type=int, default=6)
    p.add_argument("--spp-side", type=int, default=2)
    p.add_argument("--truth-side", type=int, default=16)
    p.add_argument("--frequency", type=int, default=70)
    p.add_argument("--repeat", type=int, default=5)
    p.add_argument("--out")
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

    def camera(f):
        """Frame f of the path: translation plus yaw through the Cornell view."""
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
    r_plain, r_first, r_chain = (Renderer(cfg, device=dev) for _ in range(3))
    r_first.temporal_begin()
    r_chain.temporal_begin(chain_depth=CHAIN)
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
        for r in (r_plain, r_first, r_chain):
            set_frame(r, f, a.spp_side)
        raw, _, _ = r_plain.render_adaptive(spp, spp, spp, 0.0)
        first, info_first = r_first.temporal_frame(M, spp, denoise={})
        chain, info_chain = r_chain.temporal_frame(M, spp, denoise=dict(chain_depth=CHAIN))
        # the guide pass alone: the films, the continuation rays, the wall time
        t_pass, guides, rays = {}, {}, {}
        for depth in (0, CHAIN):
            ts = []
            for _ in range(a.repeat):
                r_plain.reset_stats()
                t0 = time.perf_counter()
                guides[depth] = r_plain.render_features_chain(0, k, depth)
                ts.append((time.perf_counter() - t0) * 1e3)
            rays[depth] = r_plain.stats()["rays"]
            t_pass[depth] = min(ts)
        mask = np.any(bits(guides[0][0]) != bits(guides[CHAIN][0]), axis=1) | \
            np.any(bits(guides[0][1]) != bits(guides[CHAIN][1]), axis=1)

        def mse(x, sel):
            return float(np.mean((x[sel, :3].astype(np.float64) / np.maximum(x[sel, 3:4], 1) - truth[sel]) ** 2))
        row = {"frame": f, "pixels_changed": int(mask.sum()), "pixels_rest": int((~mask).sum()),
               "classes_first": {c: info_first[c] for c in ("reprojected", "disoccluded", "background")},
               "classes_chain": {c: info_chain[c] for c in ("reprojected", "disoccluded", "background")},
               "guide_pass_ms_depth0": round(t_pass[0], 3), "guide_pass_ms_depth4": round(t_pass[CHAIN], 3),
               "camera_rays": rays[0], "continuation_rays": rays[CHAIN] - rays[0]}
        for name, sel in (("changed", mask), ("rest", ~mask)):
            row[f"mse_{name}"] = {"raw": mse(raw, sel), "first_surface": mse(first, sel), "chain": mse(chain, sel)}
        out["frames"].append(row)
    r_first.temporal_end()
    r_chain.temporal_end()
    line = json.dumps(out)
    if a.out:
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
