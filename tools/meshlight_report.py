#!/usr/bin/env python3
"""What a mesh area light costs on the Cornell box -> one JSON line and profiles/meshlight_report.json.

usage: tools/meshlight_report.py [--res 1920x1080] [--spp 64] [--repeat 3] [--tess 46] [--out profiles/meshlight_report.json]

Needs an MI355X.  The Cornell scene (bench.py's default workload) with its ceiling light declared three ways:
    quad         RT_LIGHT_QUAD, the scene as it is: PATH with one quad light runs the simple kernels (k_path_shade);
    quad_general the same light and films, with a mirror material that no triangle uses: it switches the scene to the
                 general kernels (k_path_shade_full + k_path_nee), the ones a mesh light's scene runs — the baseline
                 that separates that switch from the cost of the mesh light itself;
    mesh_2       RT_LIGHT_MESH over the same 2 triangles: the general kernels (k_path_shade_full + k_path_nee, ML
                 instantiations), a 2-entry table;
    mesh_tess    the light's rectangle cut into --tess x --tess x 2 triangles (default 4232) behind one RT_LIGHT_MESH:
                 a binary search of 13 steps per sample — and 4266 triangles in the scene instead of 36, so the octree
                 is multi-level and every ray's traversal changes with it (the variant's octree depth is listed).
Per variant: ms per pass of --spp sample indices (wall time, default lanes; one warm-up pass, then --repeat passes taken
alternately over the variants, every figure listed), ms_shade / ms_shadow of rt_stats from one single-lane pass
(RTMI_LANES=1: with two lanes a stage's event span covers the other lane's kernels too), and the upload: the median
wall time of rt_scene_upload with the light and with an empty light list (same geometry); their difference bounds the
table build (id walk, one k_meshlight_table launch of one wave per light, one synchronisation) from above."""
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
    p.add_argument("--tess", type=int, default=46)
    p.add_argument("--out", default=str(ROOT / "profiles" / "meshlight_report.json"))
    a = p.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))
    assert 2 * a.tess * a.tess >= 4096, "--tess: the tessellated light needs at least 4096 triangles"
    LIGHT = 3                                                   # cornell_box's emissive material

    def config(name, lights=True):
        cfg = scene.cfg_cornell(res=(W, H), spp_side=16, max_depth=5)
        m = cfg.model
        if name == "mesh_tess":
            faces = np.asarray(m.positions, np.float64)[np.asarray(m.indices, np.int64)]      # object space (x, z, y)
            mats = np.asarray(m.tri_material)
            lt = faces[mats == LIGHT].reshape(-1, 3)
            gx = np.linspace(lt[:, 0].min(), lt[:, 0].max(), a.tess + 1)
            gz = np.linspace(lt[:, 1].min(), lt[:, 1].max(), a.tess + 1)
            ly = lt[0, 2]
            grid = []
            for i in range(a.tess):
                for j in range(a.tess):
                    q = [(gx[i], gz[j], ly), (gx[i + 1], gz[j], ly), (gx[i + 1], gz[j + 1], ly), (gx[i], gz[j + 1], ly)]
                    grid += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
            grid = np.array(grid)
            # the emitting side is the geometric normal's, in world space (object space with y and z swapped): down
            gw = grid[:, :, [0, 2, 1]]
            up = np.cross(gw[:, 1] - gw[:, 0], gw[:, 2] - gw[:, 0])[:, 1] > 0
            grid[up] = grid[up][:, [0, 2, 1]]
            keep = mats != LIGHT
            pos, nrm, idx = scene._flat_mesh(np.concatenate([faces[keep], grid]))
            cfg.model = scene.TriModel(pos, nrm, idx, rigid=np.eye(4), cull_backfaces=False, octree_capacity=40,
                                       tri_material=np.concatenate([mats[keep], np.full(len(grid), LIGHT)]).astype(np.int32),
                                       materials=list(m.materials), lights=list(m.lights))
        if name == "quad_general":
            cfg.model.materials = list(m.materials) + [((0.0, 0.0, 0.0), 0.0, capi.RT_MAT_MIRROR)]
        elif name != "quad":
            cfg.model.lights = [dict(type=capi.RT_LIGHT_MESH, material=LIGHT)]
        if not lights:
            cfg.model.lights = []
        return cfg

    names = ["quad", "quad_general", "mesh_2", "mesh_tess"]
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

    def upload_ms(r, name, lights):
        ts = []
        for _ in range(5):
            model = config(name, lights).model        # (the model owns the descriptor's buffers)
            d = model.desc()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = r.lib.rt_scene_upload(r.h, C.byref(d))
            ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == capi.RT_OK, r.lib.rt_last_error(r.h)
        return round(sorted(ts)[len(ts) // 2], 3)

    rs = {n: renderer(n) for n in names}
    sides = {}
    for n in names:                                   # warm-up: workspaces, code objects; the light's emitting side
        one_pass(rs[n])
        sides[n] = float(film[:, :3].sum().item())
    runs = {n: [] for n in names}
    for _ in range(a.repeat):                         # alternated: drift hits every variant alike
        for n in names:
            dt, _ = one_pass(rs[n])
            runs[n].append(round(dt * 1e3, 3))
    out = {"config": "cornell", "res": [W, H], "spp": a.spp, "library": capi.library_sha16(), "repeat": a.repeat,
           "variants": {}}
    for n in names:
        _, st = one_pass(rs[n])
        info = rs[n].octree()
        v = {"triangles": int(len(rs[n].cfg.model.indices)), "octree_depth": int(info["depth"]),
             "ms_per_pass": sorted(runs[n])[len(runs[n]) // 2], "ms_per_pass_runs": runs[n], "vs_quad": None,
             "vs_quad_general": None,
             "film_sum": sides[n],
             "counters": {k: st[k] for k in ("samples", "rays", "shadow_rays", "nee_vertices", "coop_overflows")}}
        if n.startswith("mesh"):
            tri, cdf, area = rs[n].meshlight_table(0)
            v["light_triangles"], v["light_area"] = int(len(tri)), float(area)
            with_light, without = upload_ms(rs[n], n, True), upload_ms(rs[n], n, False)
            v["upload_ms"] = {"with_light": with_light, "without_lights": without,
                              "table_build_ms_upper_bound": round(with_light - without, 3)}
        out["variants"][n] = v
    for r in rs.values():
        r.close()
    for n in names:
        r1 = renderer(n, lanes=1)
        one_pass(r1)
        dt1, st1 = one_pass(r1)
        r1.close()
        out["variants"][n]["single_lane"] = {"ms_per_pass": round(dt1 * 1e3, 3),
                                             "stage_ms": {k: round(st1[k], 3) for k in ("ms_generate", "ms_sort", "ms_trace",
                                                                                        "ms_shade", "ms_shadow", "ms_film")}}
        out["variants"][n]["vs_quad"] = round(out["variants"][n]["ms_per_pass"] / out["variants"]["quad"]["ms_per_pass"], 4)
        out["variants"][n]["vs_quad_general"] = round(out["variants"][n]["ms_per_pass"] /
                                                      out["variants"]["quad_general"]["ms_per_pass"], 4)
    # the three declarations are the same light: their films agree in the mean (not in the bits: other sample points)
    q = out["variants"]["quad"]["film_sum"]
    for n in names[1:]:
        assert abs(out["variants"][n]["film_sum"] / q - 1.0) < 0.01, (n, out["variants"][n]["film_sum"], q)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
