#!/usr/bin/env python3
"""The denoiser on the Cornell box: time and error before and after the filter -> one JSON line.

usage: tools/denoise_report.py [--res 1920x1080] [--spp-side 16] [--min 16] [--step 16] [--rel 0.1 0.05]
       tools/denoise_report.py --kernel-stats <kernel_stats.csv>
       tools/denoise_report.py --kernel-trace <kernel_trace.csv>

The first form needs an MI355X.  It renders the uniform spp-side^2 film as ground truth, then for a uniform session of
--min indices and for one session per --rel threshold: the MSE of the mean colour against the ground truth before
and after rt_adaptive_denoise.  rt_adaptive_denoise is timed (wall clock around the blocking call, best of --repeat)
on fresh sessions, where it renders the features, and once more in the same session, where it reuses them: the
difference is the feature pass.

The second form reads the per-kernel table of a `rocprofv3 --kernel-trace --stats` run of the first form and prints
the denoiser kernels' times; the third reads the run's per-dispatch trace and prints the mean time of
k_denoise_iter per step size (the iterations after a k_denoise_prepare run steps 1, 2, 4 ... in order): run it on a
trace with RTMI_DENOISE_LDS=1 and on one with RTMI_DENOISE_LDS=0 to compare the LDS tiles with plain loads."""
import argparse
import collections
import csv
import json
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
        if name.startswith("k_denoise_") or name.startswith("k_feature_"):
            ms[name] += float(r["TotalDurationNs"]) / 1e6
            calls[name] += int(r["Calls"])
    return {"kernel_ms_total": round(tot / 1e6, 3), "denoise_kernel_ms": {k: round(v, 3) for k, v in ms.items()},
            "denoise_kernel_avg_us": {k: round(1e3 * ms[k] / calls[k], 1) for k in ms}}


def per_step(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    step, dur = 0, collections.defaultdict(list)
    for r in rows:
        name = short(r["Kernel_Name"])
        if name.startswith("k_denoise_prepare"):
            step = 1
        elif name.startswith("k_denoise_iter"):
            dur[step].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            step *= 2
    return {"k_denoise_iter_us_per_step": {str(s): {"calls": len(v), "mean": round(sum(v) / len(v), 1),
                                                    "min": round(min(v), 1)} for s, v in sorted(dur.items())}}


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
    p.add_argument("--kernel-trace")
    a = p.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_share(a.kernel_stats)))
        return
    if a.kernel_trace:
        print(json.dumps(per_step(a.kernel_trace)))
        return
    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import DENOISE_DEFAULTS, Renderer

    W, H = (int(v) for v in a.res.split("x"))
    spp = a.spp_side * a.spp_side
    cfg = scene.cfg_cornell(res=(W, H), spp_side=a.spp_side)
    r = Renderer(cfg, device=torch.cuda.current_device())
    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    r.render_pass_device(0, spp, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    truth = film.cpu().numpy().astype(np.float64)
    truth = truth[:, :3] / truth[:, 3:4]

    def mse(f):
        return float(np.mean((f[:, :3].astype(np.float64) / np.maximum(f[:, 3:4], 1) - truth) ** 2))

    def session(mx, rel, floor):
        """(ms of the first denoise, ms of the second, unfiltered film, filtered film, info)"""
        r.adaptive_begin(a.mn, a.step, mx, rel, floor)
        while True:
            info = r.adaptive_step()
            if info["active_pixels"] == 0 or info["index_done"] == mx:
                break
        raw = r.adaptive_read()["film"]
        t0 = time.perf_counter()
        out = r.adaptive_denoise()
        t1 = time.perf_counter()
        r.adaptive_denoise()
        t2 = time.perf_counter()
        r.adaptive_end()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, raw, out, info

    session(a.mn, 0.0, 0.0)  # warm-up: workspaces, code objects
    out = {"config": cfg.name, "truth_spp": spp, "denoise": dict(DENOISE_DEFAULTS),
           "denoise_lds": __import__("os").environ.get("RTMI_DENOISE_LDS", "1"), "library": capi.library_sha16(),
           "cases": []}
    cases = [("uniform", a.mn, 0.0, 0.0)] + [(f"rel_error {v}", spp, v, a.abs_floor) for v in a.rel]
    for name, mx, rel, floor in cases:
        runs = [session(mx, rel, floor) for _ in range(a.repeat)]
        first, second = min(x[0] for x in runs), min(x[1] for x in runs)
        _, _, raw, den, info = runs[0]
        out["cases"].append({"case": name, "max_samples": mx, "samples": info["samples"],
                             "mean_spp": round(info["samples"] / (W * H), 2),
                             "mse_unfiltered": mse(raw), "mse_filtered": mse(den),
                             "adaptive_denoise_ms": round(first, 3), "adaptive_denoise_again_ms": round(second, 3),
                             "feature_pass_share": round(1 - second / first, 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
