#!/usr/bin/env python3
"""Temporal accumulation on the Cornell box along a camera path: pixel classes, error and time per frame -> one JSON
line.

usage: tools/temporal_report.py [--res 1920x1080] [--frames 8] [--spp-side 4] [--truth-side 16] [--out report.json]
       tools/temporal_report.py --kernel-stats <kernel_stats.csv>

The first form needs an MI355X.  The camera translates and yaws from frame to frame; every frame renders spp-side^2
uniform samples per pixel (the sampler's seed is the frame number).  Per frame it reports the three pixel counts of
rt_temporal_frame, the MSE of the mean colour against a uniform truth-side^2 film of that frame's view for the raw
frame, the frame filtered only, accumulated only, and accumulated + filtered, and the wall time (best of --repeat, the
blocking call) of rt_temporal_frame with the filter against the same frame without the temporal stage (an adaptive
session and rt_adaptive_denoise).

The second form reads the per-kernel table of a `rocprofv3 --kernel-trace --stats` run of the first form and prints the
times of the kernels the stage adds."""
import argparse
import collections
import csv
import ctypes as C
import json
import math
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def short(name):
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("::")[-1]


def kernel_share(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    ms, calls = collections.defaultdict(float), collections.defaultdict(int)
    for r in rows:
        name = short(r["Name"])
        if name.startswith("k_temporal_") or name.startswith("k_feature_") or name.startswith("k_denoise_"):
            ms[name] += float(r["TotalDurationNs"]) / 1e6
            calls[name] += int(r["Calls"])
    return {"kernel_ms_total": round(tot / 1e6, 3), "kernel_ms": {k: round(v, 3) for k, v in ms.items()},
            "kernel_calls": dict(calls), "kernel_avg_us": {k: round(1e3 * ms[k] / calls[k], 1) for k in ms}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--frames", type=int, default=8)
    p.add_argument("--spp-side", type=int, default=4)
    p.add_argument("--truth-side", type=int, default=16)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--out")
    p.add_argument("--kernel-stats")
    a = p.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_share(a.kernel_stats)))
        return
    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import DENOISE_DEFAULTS, TEMPORAL_DEFAULTS, Renderer

    W, H = (int(v) for v in a.res.split("x"))
    spp, truth_spp = a.spp_side ** 2, a.truth_side ** 2
    dev = torch.cuda.current_device()

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

    cfg = scene.cfg_cornell(res=(W, H), spp_side=a.spp_side)
    r_truth = Renderer(scene.cfg_cornell(res=(W, H), spp_side=a.truth_side), device=dev)
    r_plain, r_acc, r_both, r_time = (Renderer(cfg, device=dev) for _ in range(4))
    for r in (r_acc, r_both, r_time):
        r.temporal_begin()
    film_t = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    out = {"config": cfg.name, "res": [W, H], "frame_spp": spp, "truth_spp": truth_spp, "temporal": dict(TEMPORAL_DEFAULTS),
           "denoise": dict(DENOISE_DEFAULTS), "library": capi.library_sha16(), "frames": []}
    uniform = dict(min_samples=spp, step_samples=spp, max_samples=spp, rel_error=0.0)
    for f in range(a.frames):
        film_t.zero_()
        set_frame(r_truth, f, a.truth_side)
        r_truth.render_pass_device(0, truth_spp, film_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        truth = film_t.cpu().numpy().astype(np.float64)
        truth = truth[:, :3] / truth[:, 3:4]

        def mse(x):
            return float(np.mean((x[:, :3].astype(np.float64) / np.maximum(x[:, 3:4], 1) - truth) ** 2))
        M = scene.world_to_film(camera(f))
        for r in (r_plain, r_acc, r_both, r_time):
            set_frame(r, f, a.spp_side)
        raw, mom, _ = r_plain.render_adaptive(**uniform)
        filt = r_plain.denoise(raw, mom, r_plain.render_features(0, DENOISE_DEFAULTS["feature_samples"]))
        acc, info = r_acc.temporal_frame(M, spp)
        both, info_b = r_both.temporal_frame(M, spp, denoise={})
        assert info == info_b
        t_frame, t_plain = [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            r_time.temporal_frame(M, spp, denoise={})
            t1 = time.perf_counter()
            r_plain.render_denoised(spp, spp, spp, 0.0)
            t2 = time.perf_counter()
            t_frame.append((t1 - t0) * 1e3)
            t_plain.append((t2 - t1) * 1e3)
        out["frames"].append({"frame": f, **info, "mean_history": round(float(acc[:, 3].mean()), 2),
                              "mse_raw": mse(raw), "mse_filtered": mse(filt), "mse_accumulated": mse(acc),
                              "mse_accumulated_filtered": mse(both), "temporal_frame_ms": round(min(t_frame), 3),
                              "plain_frame_ms": round(min(t_plain), 3)})
    for r in (r_acc, r_both, r_time):
        r.temporal_end()
    line = json.dumps(out)
    if a.out:
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
