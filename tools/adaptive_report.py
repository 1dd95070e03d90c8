#!/usr/bin/env python3
"""Adaptive sampling against uniform rendering on the Cornell box -> one JSON line.

usage: tools/adaptive_report.py [--res 1920x1080] [--spp-side 16] [--min 16] [--step 16] [--rel 0.1 0.05]
       tools/adaptive_report.py --kernel-stats <kernel_stats.csv>

The first form needs an MI355X.  It renders indices [0, spp) uniformly into a device film (rt_render_pass_device),
then runs adaptive sessions (begin, step until done, end; film and moments stay on the device): one at rel_error 0
with abs_floor 0, where no block ever converges (a black block is 0 / 0), so every pixel takes every index and the
ratio to the uniform time is the overhead of the moment film, the error estimate and the compaction; then one at
each --rel threshold with --abs-floor.  Times are wall clock around synchronised calls, the best of --repeat.

The second form reads the per-kernel table of a `rocprofv3 --kernel-trace --stats` run of the first form and prints
the share of kernel time spent in the error and compaction kernels (k_adaptive_*)."""
import argparse
import csv
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def kernel_share(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    ad, calls = {}, {}
    for r in rows:
        name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1]
        if name.startswith("k_adaptive_"):
            ad[name] = ad.get(name, 0.0) + float(r["TotalDurationNs"])
            calls[name] = calls.get(name, 0) + int(r["Calls"])
    return {"kernel_ms_total": round(tot / 1e6, 3), "adaptive_kernel_ms": {k: round(v / 1e6, 3) for k, v in ad.items()},
            "adaptive_kernel_avg_us": {k: round(ad[k] / calls[k] / 1e3, 1) for k in ad},
            "adaptive_kernel_share": round(sum(ad.values()) / tot, 6) if tot else None}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--spp-side", type=int, default=16)
    p.add_argument("--min", type=int, default=16, dest="mn")
    p.add_argument("--step", type=int, default=16)
    p.add_argument("--rel", type=float, nargs="*", default=[0.1, 0.05])
    p.add_argument("--abs-floor", type=float, default=1e-3)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--kernel-stats")
    a = p.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_share(a.kernel_stats)))
        return
    import torch

    from computational_ray_tracer_amd import scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))
    spp = a.spp_side * a.spp_side
    cfg = scene.cfg_cornell(res=(W, H), spp_side=a.spp_side)
    r = Renderer(cfg, device=torch.cuda.current_device())
    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def uniform():
        film.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r.render_pass_device(0, spp, film.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def session(rel, floor):
        r.adaptive_begin(a.mn, a.step, spp, rel, floor)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        active = []
        while True:
            info = r.adaptive_step()  # (blocks until the step's counts are read)
            active.append(info["active_pixels"])
            if info["active_pixels"] == 0 or info["index_done"] == spp:
                break
        ms = (time.perf_counter() - t0) * 1e3
        r.adaptive_end()
        return ms, info, active

    uniform()  # warm-up: workspaces, code objects
    uni_ms = min(uniform() for _ in range(a.repeat))
    out = {"config": cfg.name, "spp": spp, "min_samples": a.mn, "step_samples": a.step,
           "uniform": {"samples": W * H * spp, "ms": round(uni_ms, 2)}, "adaptive": []}
    for rel, floor in [(0.0, 0.0)] + [(v, a.abs_floor) for v in a.rel]:
        best = None
        for _ in range(a.repeat):
            ms, info, active = session(rel, floor)
            if best is None or ms < best[0]:
                best = (ms, info, active)
        ms, info, active = best
        out["adaptive"].append({"rel_error": rel, "abs_floor": floor, "samples": info["samples"], "ms": round(ms, 2),
                                "iterations": info["iterations"], "index_done": info["index_done"],
                                "active_pixels_per_iteration": active,
                                "sample_ratio_to_uniform": round(info["samples"] / (W * H * spp), 4),
                                "ms_ratio_to_uniform": round(ms / uni_ms, 4)})
    out["overhead_rel0"] = out["adaptive"][0]["ms_ratio_to_uniform"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
