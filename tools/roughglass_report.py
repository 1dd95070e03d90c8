#!/usr/bin/env python3
"""What rough glass costs on the Cornell box -> one JSON line and profiles/roughglass_report.json.

usage: tools/roughglass_report.py [--res 1920x1080] [--spp 64] [--repeat 3] [--out profiles/roughglass_report.json]

Needs an MI355X.  The report scene of tools/rough_report.py (the Cornell geometry under RT_INTEGRATOR_PATH_MIS with a second
light, one RT_LIGHT_DISTANT, so that both variants run the general kernels k_path_shade_full + k_path_nee):
    rough        the floor at alpha 0.1 and the two blocks at alpha 0.4 as RT_MAT_ROUGH (the white wall's sigmoid): RGH
                 level 1;
    roughglass   the same floor, the two blocks as RT_MAT_ROUGH_DIELECTRIC (eta 1.5, alpha 0.2): RGH level 3.  Its paths
                 enter the blocks and leave them again, so it traces other rays than `rough` does: the counters say how
                 many, and the per-stage times are per pass, not per ray.
Per variant: ms per pass of --spp sample indices (wall time, default lanes; one warm-up pass, then --repeat passes taken
alternately over the variants, every figure listed), rt_stats' counters, the level-1, level-2 and level-3 launch counts of
the last pass (rt_debug_rough_stats, rt_debug_conductor_stats, rt_debug_roughglass_stats) and, from one single-lane pass (RTMI_LANES=1: with two lanes a
stage's event span covers the other lane's kernels too), rt_stats' stage times."""
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
    p.add_argument("--out", default=str(ROOT / "profiles" / "roughglass_report.json"))
    a = p.parse_args()

    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))
    names = ["rough", "roughglass"]

    def config(name):
        cfg = scene.cfg_cornell(res=(W, H), spp_side=16, max_depth=5)
        cfg.integrator.kind = capi.RT_INTEGRATOR_PATH_MIS
        m = cfg.model
        m.lights = list(m.lights) + [dict(type=capi.RT_LIGHT_DISTANT, dir=(0.2, 0.3, -1.0), scale=2.0)]
        white = tuple(m.materials[0][0])
        mats = [tuple(x) for x in m.materials]
        if name == "rough":
            mats += [scene.rough(white, 0.1), scene.rough(white, 0.4)]
        else:
            mats += [scene.rough(white, 0.1), scene.rough_glass(1.5, 0.2)]
        tm = np.array(m.tri_material, np.int32)
        tm[0:2] = len(mats) - 2            # the floor
        tm[12:36] = len(mats) - 1          # the short and the tall block
        m.materials, m.tri_material = mats, tm
        return cfg

    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def renderer(name, lanes=None):
        old = os.environ.get("RTMI_LANES")
        if lanes is not None:
            os.environ["RTMI_LANES"] = str(lanes)
        try:
            return Renderer(config(name), device=torch.cuda.current_device())
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
    out = {"config": "cornell geometry, PATH_MIS, quad + distant light", "res": [W, H], "spp": a.spp,
           "library": capi.library_sha16(), "repeat": a.repeat, "variants": {}}
    for n in names:
        _, st = one_pass(rs[n])
        out["variants"][n] = {
            "ms_per_pass": sorted(runs[n])[len(runs[n]) // 2], "ms_per_pass_runs": runs[n], "vs_rough": None,
            "film_sum": sums[n], "rgh_launches": rs[n].rough_launches(), "conductor_launches": rs[n].conductor_launches(),
            "roughglass_launches": rs[n].roughglass_launches(),
            "counters": {k: st[k] for k in ("samples", "rays", "hits", "shadow_rays", "nee_vertices", "coop_overflows")}}
    for r in rs.values():
        r.close()
    for n in names:
        r1 = renderer(n, lanes=1)
        one_pass(r1)
        dt1, st1 = one_pass(r1)
        r1.close()
        v = out["variants"][n]
        v["single_lane"] = {"ms_per_pass": round(dt1 * 1e3, 3),
                            "stage_ms": {k: round(st1[k], 3) for k in ("ms_generate", "ms_sort", "ms_trace", "ms_shade",
                                                                       "ms_shadow", "ms_film")}}
        v["vs_rough"] = round(v["ms_per_pass"] / out["variants"]["rough"]["ms_per_pass"], 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
