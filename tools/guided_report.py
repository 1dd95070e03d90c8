#!/usr/bin/env python3
"""Guided against unguided temporal frames on the Cornell box along a camera path: samples, iterations, time, pixel
classes and error per frame -> one JSON line.

usage: tools/guided_report.py [--res 1920x1080] [--frames 8] [--spp-side 8] [--truth-side 16] [--repeat 3]
                              [--min-samples 4] [--step-samples 4] [--max-samples 64] [--rel-error 0.05]
                              [--abs-floor 1e-3] [--no-truth] [--out report.json]
       tools/guided_report.py --kernel-stats <kernel_stats.csv>

The first form needs an MI355X.  The camera path is tools/temporal_report.py's (translation (8, -3, 6) and 1 degree of
yaw per frame; the sampler's seed is the frame number).  Two temporal sessions with the same descriptors, one calling
rt_temporal_frame and one rt_temporal_frame_guided, both filtered with the default denoise descriptor, walk the path
--repeat times with rt_temporal_reset in between, alternating frame by frame (unguided first): every walk renders the
same samples, so the counts and errors are the first walk's and the wall time of a frame (the blocking call) is the best
of the walks.  Per frame and session: the samples rendered (the guided frame's session_info; the rt_get_stats delta of
both, with whether the two agree), the session's iterations (guided: session_info; unguided: an adaptive session of the
same descriptor on a third renderer), the pixel classes, the mean history length, and the MSE of the
frame's output (accumulated + filtered) against a uniform truth-side^2 film of the frame's view.

The second form reads the per-kernel table of a `rocprofv3 --kernel-trace --stats` run of the first form and prints the
per-launch times of the kernels the guided estimate adds beside those of the kernels they stand in for."""
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
        if name.startswith("k_temporal_") or name.startswith("k_adaptive_"):
            ms[name] += float(r["TotalDurationNs"]) / 1e6
            calls[name] += int(r["Calls"])
    return {"kernel_ms_total": round(tot / 1e6, 3), "kernel_ms": {k: round(v, 3) for k, v in ms.items()},
            "kernel_calls": dict(calls), "kernel_avg_us": {k: round(1e3 * ms[k] / calls[k], 1) for k in ms}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--frames", type=int, default=8)
    p.add_argument("--spp-side", type=int, default=8)
    p.add_argument("--truth-side", type=int, default=16)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--min-samples", type=int, default=4)
    p.add_argument("--step-samples", type=int, default=4)
    p.add_argument("--max-samples", type=int, default=64)
    p.add_argument("--rel-error", type=float, default=0.05)
    p.add_argument("--abs-floor", type=float, default=1e-3)
    p.add_argument("--no-truth", action="store_true")
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
    truth_spp = a.truth_side ** 2
    assert a.max_samples <= a.spp_side ** 2, "max_samples exceeds the sampler's samples per pixel"
    dev = torch.cuda.current_device()
    adaptive = dict(min_samples=a.min_samples, step_samples=a.step_samples, max_samples=a.max_samples,
                    rel_error=a.rel_error, abs_floor=a.abs_floor)

    def camera(f):
        yaw = math.radians(1.0 * f)
        return scene.PerspectiveCamera(near=1.0, far=5000.0, fov=62.0,
                                       position=(278.0 + 8.0 * f, 273.0 - 3.0 * f, -800.0 + 6.0 * f),
                                       look=(math.sin(yaw), 0.0, math.cos(yaw)), right=(1, 0, 0), worldup=(0, 1, 0),
                                       res=(W, H), lens_radius=0.0, focal_distance=0.0, aspect_fix=True)

    def set_frame(r, f, side):
        r.set_camera(camera(f))
        r._chk("rt_sampler_set", r.lib.rt_sampler_set(r.h, C.byref(scene.StratifiedSampler(side, side, True, f).desc())))

    cfg = scene.cfg_cornell(res=(W, H), spp_side=a.spp_side)
    sessions = {"unguided": Renderer(cfg, device=dev), "guided": Renderer(cfg, device=dev)}
    r_plain = Renderer(cfg, device=dev)
    for r in sessions.values():
        r.temporal_begin()
    out = {"config": cfg.name, "res": [W, H], "sampler_spp": a.spp_side ** 2, "truth_spp": None if a.no_truth else truth_spp,
           "adaptive": adaptive, "temporal": dict(TEMPORAL_DEFAULTS), "denoise": dict(DENOISE_DEFAULTS),
           "repeat": a.repeat, "library": capi.library_sha16(), "frames": []}
    truths = []
    if not a.no_truth:
        r_truth = Renderer(scene.cfg_cornell(res=(W, H), spp_side=a.truth_side), device=dev)
        film_t = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
        for f in range(a.frames):
            film_t.zero_()
            set_frame(r_truth, f, a.truth_side)
            r_truth.render_pass_device(0, truth_spp, film_t.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            t = film_t.cpu().numpy().astype(np.float64)
            truths.append(t[:, :3] / t[:, 3:4])
        r_truth.close()
    rows = [{"frame": f} for f in range(a.frames)]
    for walk in range(a.repeat):
        for r in sessions.values():
            r.temporal_reset()
        for f in range(a.frames):
            M = scene.world_to_film(camera(f))
            for which, r in sessions.items():
                set_frame(r, f, a.spp_side)
                r.reset_stats()
                t0 = time.perf_counter()
                film, info = r.temporal_frame(M, denoise={}, guided=which == "guided", **adaptive)
                ms = (time.perf_counter() - t0) * 1e3
                row = rows[f].setdefault(which, {"ms": []})
                row["ms"].append(round(ms, 3))
                if walk:
                    continue
                row["stats_samples"] = int(r.stats()["samples"])
                row["mean_history"] = round(float(film[:, 3].mean()), 2)
                row.update({k: info[k] for k in ("frames", "reprojected", "disoccluded", "background")})
                if which == "guided":
                    row["session"] = info["session"]
                else:
                    set_frame(r_plain, f, a.spp_side)
                    row["session"] = r_plain.render_adaptive(**adaptive)[2]
                row["samples"] = int(row["session"]["samples"])
                row["samples_agree"] = row["samples"] == row["stats_samples"]
                if truths:
                    row["mse_accumulated_filtered"] = float(np.mean(
                        (film[:, :3].astype(np.float64) / np.maximum(film[:, 3:4], 1) - truths[f]) ** 2))
    for row in rows:
        for which in sessions:
            row[which]["best_ms"] = min(row[which]["ms"])
        out["frames"].append(row)
    for r in sessions.values():
        r.temporal_end()
    line = json.dumps(out)
    if a.out:
        Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
