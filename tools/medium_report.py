#!/usr/bin/env python3
"""What an absorbing medium costs on the Cornell box -> one JSON line and profiles/medium_report.json.

usage: tools/medium_report.py [--res 1920x1080] [--spp 64] [--repeat 3] [--out profiles/medium_report.json]
       tools/medium_report.py --trace-variant rough_medium          (one warm-up and one pass: the program to put behind
                                                                     `rocprofv3 --kernel-trace --stats --`)
       tools/medium_report.py --merge-trace DIR                      (adds k_medium_absorb's row of the kernel statistics
                                                                     found under DIR to the JSON)

Needs an MI355X.  §3m's report scene (tools/roughglass_report.py: the Cornell geometry under RT_INTEGRATOR_PATH_MIS with a
second light, one RT_LIGHT_DISTANT, the floor rough at alpha 0.1) with its two blocks as glass, first smooth
(RT_MAT_DIELECTRIC, eta 1.5), then rough (RT_MAT_ROUGH_DIELECTRIC, eta 1.5, alpha 0.2), each without and with a medium on
the blocks' material whose sigma_a times the blocks' smallest edge is 1 (S = the sigmoid of rgb (0.2, 0.6, 0.9), the mean
of S over 360-830 nm folded into sigma):
    smooth, smooth_medium, rough, rough_medium
Per variant: ms per pass of --spp sample indices (wall time, default lanes; one warm-up pass, then --repeat passes taken
alternately over the variants, every figure listed, the median reported), rt_stats' counters, the absorb stage's launches
and attenuated segments of the last pass (rt_debug_medium_stats) and, from one single-lane pass (RTMI_LANES=1: with two
lanes a stage's event span covers the other lane's kernels too), rt_stats' stage times (the absorb stage is timed into
ms_shade)."""
import argparse
import csv
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

NAMES = ["smooth", "smooth_medium", "rough", "rough_medium"]


def merge_trace(out_path, trace_dir):
    rows = []
    for f in sorted(Path(trace_dir).rglob("*kernel_stats.csv")):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r.get("Name") or r.get("KernelName") or ""
                if "k_medium_absorb" in name:
                    rows.append({"file": f.name, "calls": int(r["Calls"]), "total_ns": int(float(r["TotalDurationNs"])),
                                 "average_ns": float(r["AverageNs"]), "min_ns": int(float(r["MinNs"])),
                                 "max_ns": int(float(r["MaxNs"])), "percentage": float(r["Percentage"])})
    if not rows:
        raise SystemExit(f"no k_medium_absorb row in any *kernel_stats.csv under {trace_dir}")
    out = json.loads(Path(out_path).read_text())
    out["kernel_trace"] = {"tool": "rocprofv3 --kernel-trace --stats", "k_medium_absorb": rows}
    Path(out_path).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["kernel_trace"]))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--spp", type=int, default=64)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--out", default=str(ROOT / "profiles" / "medium_report.json"))
    p.add_argument("--trace-variant", choices=NAMES)
    p.add_argument("--merge-trace")
    a = p.parse_args()
    if a.merge_trace:
        return merge_trace(a.out, a.merge_trace)

    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))

    def config(name):
        cfg = scene.cfg_cornell(res=(W, H), spp_side=16, max_depth=5)
        cfg.integrator.kind = capi.RT_INTEGRATOR_PATH_MIS
        m = cfg.model
        m.lights = list(m.lights) + [dict(type=capi.RT_LIGHT_DISTANT, dir=(0.2, 0.3, -1.0), scale=2.0)]
        white = tuple(m.materials[0][0])
        mats = [tuple(x) for x in m.materials]
        glass = ((0.0, 0.0, 0.0), 0.0, capi.RT_MAT_DIELECTRIC, 1.5) if name.startswith("smooth") else scene.rough_glass(1.5, 0.2)
        mats += [scene.rough(white, 0.1), glass]
        tm = np.array(m.tri_material, np.int32)
        tm[0:2] = len(mats) - 2            # the floor
        tm[12:36] = len(mats) - 1          # the short and the tall block
        m.materials, m.tri_material = mats, tm
        media = None
        if name.endswith("_medium"):
            pos = np.asarray(m.positions, np.float64)[np.asarray(m.indices, np.int64)[12:24].reshape(-1)]   # the short block
            edge = float((pos.max(axis=0) - pos.min(axis=0)).min())
            med = scene.absorbing((0.2, 0.6, 0.9), 1.0)
            lam = np.linspace(360.0, 830.0, 8, dtype=np.float32)[None, :]
            s_mean = float(-np.log(scene.medium_transmittance(med, lam, [1.0])).mean())
            med.sigma = 1.0 / (edge * s_mean)
            media = [None] * (len(mats) - 1) + [med]
        return cfg, media

    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def renderer(name, lanes=None):
        old = os.environ.get("RTMI_LANES")
        if lanes is not None:
            os.environ["RTMI_LANES"] = str(lanes)
        try:
            cfg, media = config(name)
            r = Renderer(cfg, device=torch.cuda.current_device())
            r.set_media(media)
            return r
        finally:
            if lanes is not None:
                os.environ.pop("RTMI_LANES", None) if old is None else os.environ.__setitem__("RTMI_LANES", old)

    def one_pass(r):
        film.zero_()
        torch.cuda.synchronize()
        r.reset_stats()
        t0 = time.perf_counter()
        r.render_pass_device(0, a.spp, film.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r.stats()

    if a.trace_variant:
        r = renderer(a.trace_variant)
        one_pass(r)
        dt, _ = one_pass(r)
        print(json.dumps({"variant": a.trace_variant, "ms_per_pass": round(dt * 1e3, 3), "medium_stats": r.medium_stats()}))
        r.close()
        return

    rs = {n: renderer(n) for n in NAMES}
    sums = {}
    for n in NAMES:                                   # warm-up: workspaces, code objects
        one_pass(rs[n])
        sums[n] = [float(v) for v in film[:, :3].sum(dim=0).tolist()]
    runs = {n: [] for n in NAMES}
    for _ in range(a.repeat):                         # alternated: drift hits every variant alike
        for n in NAMES:
            dt, _ = one_pass(rs[n])
            runs[n].append(round(dt * 1e3, 3))
    out = {"config": "cornell geometry, PATH_MIS, quad + distant light, the two blocks glass", "res": [W, H], "spp": a.spp,
           "library": capi.library_sha16(), "repeat": a.repeat, "variants": {}}
    for n in NAMES:
        _, st = one_pass(rs[n])
        launches, segments = rs[n].medium_stats()
        out["variants"][n] = {
            "ms_per_pass": sorted(runs[n])[len(runs[n]) // 2], "ms_per_pass_runs": runs[n], "vs_no_medium": None,
            "film_sum_rgb": sums[n], "absorb_launches": launches, "absorbed_segments": segments,
            "roughglass_launches": rs[n].roughglass_launches(),
            "counters": {k: st[k] for k in ("samples", "rays", "hits", "shadow_rays", "nee_vertices", "coop_overflows")}}
    for r in rs.values():
        r.close()
    for n in NAMES:
        r1 = renderer(n, lanes=1)
        one_pass(r1)
        dt1, st1 = one_pass(r1)
        r1.close()
        v = out["variants"][n]
        v["single_lane"] = {"ms_per_pass": round(dt1 * 1e3, 3),
                            "stage_ms": {k: round(st1[k], 3) for k in ("ms_generate", "ms_sort", "ms_trace", "ms_shade",
                                                                       "ms_shadow", "ms_film")}}
        v["vs_no_medium"] = round(v["ms_per_pass"] / out["variants"][n.replace("_medium", "")]["ms_per_pass"], 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
