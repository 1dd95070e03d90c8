#!/usr/bin/env python3
"""What the environment light costs on the Cornell box -> one JSON line and profiles/envlight_report.json.

usage: tools/envlight_report.py [--res 1920x1080] [--spp 64] [--repeat 3] [--out profiles/envlight_report.json]

Needs an MI355X.  The Cornell geometry (bench.py's default workload) with its light list replaced three ways, all of
them on the general kernels (k_path_shade_full + k_path_nee):
    distant        one RT_LIGHT_DISTANT: the comparison — one light, one shadow ray per vertex, no table, no miss stage;
    env_1x1        no light records, a 1 x 1 environment map: the TL = 2 instantiations, a one-entry table, k_env_miss;
    env_1024x512   the same with a 1024 x 512 HDR map (a smooth sky with a small bright sun): 19 search steps per sample.
Per variant: ms per pass of --spp sample indices (wall time, default lanes; one warm-up pass, then --repeat passes taken
alternately over the variants, every figure listed) and, from one single-lane pass (RTMI_LANES=1: with two lanes a
stage's event span covers the other lane's kernels too), rt_stats' stage times and the miss stage's own time
(rt_debug_env_stats; rt_stats.ms_shade includes it).  For the large map also the wall time of rt_scene_set_environment
(copy, k_env_bake, k_env_table, the light list), median of 5."""
import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--spp", type=int, default=64)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--out", default=str(ROOT / "profiles" / "envlight_report.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))

    def sky(w, h):
        """A smooth gradient with a sun 200 times brighter on a few texels (HDR: values above 1)."""
        y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        m = np.stack([0.25 + 0.2 * x / w, 0.3 + 0.2 * y / h, 0.5 + 0 * x], -1).astype(np.float32)
        cy, cx = int(0.55 * h), int(0.6 * w)
        m[cy - h // 128:cy + h // 128 + 1, cx - w // 256:cx + w // 256 + 1] = 60.0
        return m

    envs = {"env_1x1": scene.Environment(np.full((1, 1, 3), 0.5, np.float32)),
            "env_1024x512": scene.Environment(sky(1024, 512))}
    names = ["distant", "env_1x1", "env_1024x512"]

    def config(name):
        cfg = scene.cfg_cornell(res=(W, H), spp_side=16, max_depth=5)
        cfg.model.lights = [dict(type=capi.RT_LIGHT_DISTANT, dir=(0.2, 0.3, -1.0), scale=2.0)] if name == "distant" else []
        return cfg

    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def renderer(name, lanes=None):
        old = os.environ.get("RTMI_LANES")
        if lanes is not None:
            os.environ["RTMI_LANES"] = str(lanes)
        try:
            r = Renderer(config(name), device=torch.cuda.current_device())
        finally:
            if lanes is not None:
                os.environ.pop("RTMI_LANES", None) if old is None else os.environ.__setitem__("RTMI_LANES", old)
        if name in envs:
            r.set_environment(envs[name])
        return r

    def one_pass(r):
        film.zero_()
        torch.cuda.synchronize()
        r.reset_stats()
        t0 = time.perf_counter()
        r.render_pass_device(0, a.spp, film.data_ptr(), stream.cuda_stream)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r.stats()

    rs = {n: renderer(n) for n in names}
    sums = {}
    for n in names:                                   # warm-up: workspaces, code objects
        one_pass(rs[n])
        sums[n] = float(film[:, :3].sum().item())
    runs = {n: [] for n in names}
    for _ in range(a.repeat):                         # alternated: drift hits every variant alike
        for n in names:
            dt, _ = one_pass(rs[n])
            runs[n].append(round(dt * 1e3, 3))
    out = {"config": "cornell geometry", "res": [W, H], "spp": a.spp, "library": capi.library_sha16(), "repeat": a.repeat,
           "variants": {}}
    for n in names:
        _, st = one_pass(rs[n])
        v = {"ms_per_pass": sorted(runs[n])[len(runs[n]) // 2], "ms_per_pass_runs": runs[n], "vs_distant": None,
             "film_sum": sums[n],
             "counters": {k: st[k] for k in ("samples", "rays", "hits", "shadow_rays", "nee_vertices", "coop_overflows")}}
        if n == "env_1024x512":
            ts = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rs[n].set_environment(envs[n])
                ts.append(round((time.perf_counter() - t0) * 1e3, 3))
            v["set_environment_ms"] = {"median": sorted(ts)[len(ts) // 2], "runs": ts}
        out["variants"][n] = v
    for r in rs.values():
        r.close()
    for n in names:
        r1 = renderer(n, lanes=1)
        one_pass(r1)
        dt1, st1 = one_pass(r1)
        ms_miss = r1.env_miss_ms() if n in envs else 0.0
        r1.close()
        v = out["variants"][n]
        v["single_lane"] = {"ms_per_pass": round(dt1 * 1e3, 3),
                            "stage_ms": {k: round(st1[k], 3) for k in ("ms_generate", "ms_sort", "ms_trace", "ms_shade",
                                                                       "ms_shadow", "ms_film")},
                            "ms_env_miss": round(ms_miss, 3)}
        v["vs_distant"] = round(v["ms_per_pass"] / out["variants"]["distant"]["ms_per_pass"], 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
