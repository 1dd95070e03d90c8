#!/usr/bin/env python3
"""What an albedo texture costs on CFG3's blob -> one JSON line and profiles/texture_report.json.

usage: tools/texture_report.py [--res 1920x1080] [--spp 512] [--repeat 3] [--out profiles/texture_report.json]

Needs an MI355X.  CFG3's scene (the 98k-triangle procedural mesh in the Cornell box, bench.py --config cfg3) rendered
three ways:
    untextured   the scene as it is: PATH with one quad light runs k_path_shade, the path every earlier build took;
    tex_1x1      every diffuse material bound to a 1 x 1 texture (a grey, a red, a green): the cost of the switch
                 to the general kernels (k_path_shade_full + k_path_nee, TEX instantiations) plus a fetch that always
                 hits the same 16 bytes;
    tex_1024     the white material (walls and mesh) bound to a seeded 1024 x 1024 texture, uv a spherical map of the
                 vertex positions about the scene's centre: scattered fetches over 16 MiB of texels.
Per variant: Msamples/s over the wall time of whole passes (default lanes; one warm-up pass, then --repeat passes taken
alternately over the variants, every figure listed) and the rt_stats stage times of one single-lane pass
(RTMI_LANES=1: with two lanes a stage's event span covers the other lane's kernels too)."""
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
    p.add_argument("--spp", type=int, default=512)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--frequency", type=int, default=70)
    p.add_argument("--out", default=str(ROOT / "profiles" / "texture_report.json"))
    a = p.parse_args()
    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi, scene
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))
    cfg = scene.cfg3_blob(res=(W, H), spp_side=16, max_depth=5, frequency=a.frequency)
    cfg.sampler = scene.StratifiedSampler(32, 16, True, 0)     # bench.py --config cfg3: 512 spp
    assert a.spp <= cfg.sampler.spp()
    m = cfg.model
    tri = np.asarray(m.indices, np.int64)

    def variant(name):
        """(textures, material_texture, tri_texcoords) or None"""
        if name == "untextured":
            return None
        nt = len(tri)
        if name == "tex_1x1":
            # (a material's sigmoid does not give its RGB back: a mid grey, a red and a green stand in)
            cols = [(186, 186, 186), (161, 17, 13), (36, 115, 23)]
            tex = [scene.Texture(np.array(c, np.uint8).reshape(1, 1, 3)) for c in cols]
            return tex, [0, 1, 2, -1], np.full((nt, 3, 2), 0.5, np.float32)
        rng = np.random.default_rng(1024)
        tex = [scene.Texture(rng.integers(30, 226, (1024, 1024, 3)).astype(np.uint8), wrap="repeat")]
        pos = np.asarray(m.positions, np.float64)
        d = pos - pos.mean(axis=0)
        d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
        uv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], -1)
        return tex, [0, -1, -1, -1], uv.astype(np.float32)[tri]

    names = ["untextured", "tex_1x1", "tex_1024"]
    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()

    def renderer(name, lanes=None):
        old = os.environ.get("RTMI_LANES")
        if lanes is not None:
            os.environ["RTMI_LANES"] = str(lanes)
        try:
            r = Renderer(cfg, device=torch.cuda.current_device())
        finally:
            if lanes is not None:
                os.environ.pop("RTMI_LANES", None) if old is None else os.environ.__setitem__("RTMI_LANES", old)
        v = variant(name)
        if v is not None:
            r.set_textures(*v)
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
    for n in names:                                   # warm-up: workspaces, code objects
        one_pass(rs[n])
    runs = {n: [] for n in names}
    for _ in range(a.repeat):                         # alternated: drift hits every variant alike
        for n in names:
            dt, st = one_pass(rs[n])
            runs[n].append(round(st["samples"] / dt / 1e6, 3))
    counters = {n: one_pass(rs[n])[1] for n in names}
    for r in rs.values():
        r.close()
    out = {"config": f"cfg3_blob{len(tri) - 12}", "res": [W, H], "spp": a.spp, "triangles": int(len(tri)), "library": capi.library_sha16(),
           "repeat": a.repeat, "variants": {}}
    for n in names:
        r1 = renderer(n, lanes=1)
        one_pass(r1)
        dt1, st1 = one_pass(r1)
        r1.close()
        ms = sorted(runs[n])
        out["variants"][n] = {
            "msamples_per_s": ms[len(ms) // 2], "msamples_per_s_runs": runs[n],
            "vs_untextured": None,
            "single_lane": {"msamples_per_s": round(st1["samples"] / dt1 / 1e6, 3),
                            "stage_ms": {k: round(st1[k], 3) for k in ("ms_generate", "ms_sort", "ms_trace", "ms_shade",
                                                                       "ms_shadow", "ms_film")}},
            "counters": {k: counters[n][k] for k in ("samples", "rays", "shadow_rays", "nee_vertices", "coop_overflows")}}
    base = out["variants"]["untextured"]["msamples_per_s"]
    for n in names:
        out["variants"][n]["vs_untextured"] = round(out["variants"][n]["msamples_per_s"] / base, 4)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
