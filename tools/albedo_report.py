#!/usr/bin/env python3
"""Albedo demodulation on CFG3's textured blob: error and time with and without it -> one JSON line and
profiles/albedo_report.json.

usage: tools/albedo_report.py [--res 1920x1080] [--spp 16] [--truth-spp 256] [--repeat 3] [--out profiles/albedo_report.json]
       tools/albedo_report.py --time-only [--plain-only]

Needs an MI355X.  The scene is tools/texture_report.py's tex_1024 variant: CFG3 (the 98k-triangle procedural mesh in the
Cornell box) with the white material bound to a seeded 1024 x 1024 texture.  A uniform --truth-spp film is the ground
truth; a uniform session of --spp indices gives the MSE of the mean colour unfiltered, after rt_adaptive_denoise and
after rt_adaptive_denoise_albedo.  Both calls are timed (wall clock around the blocking call, best of --repeat) on fresh
sessions, where they render their guide films, and once more in the same session, where they reuse them; the bake of
the 1024^2 texels' albedo table is the first demodulating call of a context minus a later first call.

--time-only prints the timings alone; with --plain-only it touches nothing but rt_adaptive_denoise, so the same file runs
against an older build of the library for a before/after comparison on one machine."""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
if "computational_ray_tracer_amd" not in sys.modules:   # (a caller may have put another build's package first)
    sys.path.insert(0, str(ROOT))


def textured_cfg3(W, H, frequency=70):
    """(cfg, (textures, material_texture, tri_texcoords)) of texture_report.py's tex_1024 variant."""
    import numpy as np

    from computational_ray_tracer_amd import scene
    cfg = scene.cfg3_blob(res=(W, H), spp_side=16, max_depth=5, frequency=frequency)
    cfg.sampler = scene.StratifiedSampler(32, 16, True, 0)     # bench.py --config cfg3: 512 spp
    m = cfg.model
    tri = np.asarray(m.indices, np.int64)
    rng = np.random.default_rng(1024)
    tex = [scene.Texture(rng.integers(30, 226, (1024, 1024, 3)).astype(np.uint8), wrap="repeat")]
    pos = np.asarray(m.positions, np.float64)
    d = pos - pos.mean(axis=0)
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-12)
    uv = np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], -1)
    return cfg, (tex, [0, -1, -1, -1], uv.astype(np.float32)[tri])


def session(r, spp, demodulate):
    """A uniform session of spp indices: (ms of the first filter call, ms of the second, unfiltered film, filtered)."""
    kw = dict(demodulate=True) if demodulate else {}
    r.adaptive_begin(spp, spp, spp, 0.0, 0.0)
    r.adaptive_step()
    raw = r.adaptive_read()["film"]
    t0 = time.perf_counter()
    out = r.adaptive_denoise(**kw)
    t1 = time.perf_counter()
    r.adaptive_denoise(**kw)
    t2 = time.perf_counter()
    r.adaptive_end()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, raw, out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", default="1920x1080")
    p.add_argument("--spp", type=int, default=16)
    p.add_argument("--truth-spp", type=int, default=256)
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--frequency", type=int, default=70)
    p.add_argument("--time-only", action="store_true")
    p.add_argument("--plain-only", action="store_true")
    p.add_argument("--out", default=str(ROOT / "profiles" / "albedo_report.json"))
    a = p.parse_args()
    import numpy as np
    import torch

    from computational_ray_tracer_amd import capi
    from computational_ray_tracer_amd.renderer import Renderer

    W, H = (int(v) for v in a.res.split("x"))
    cfg, tex = textured_cfg3(W, H, a.frequency)
    r = Renderer(cfg, device=torch.cuda.current_device())
    r.set_textures(*tex)
    out = {"config": cfg.name, "res": [W, H], "spp": a.spp, "texture": "1024x1024 on the white material",
           "library": capi.library_sha16()}
    session(r, a.spp, False)                               # warm-up: workspaces, code objects
    runs = [session(r, a.spp, False) for _ in range(a.repeat)]
    out["adaptive_denoise_ms"] = round(min(x[0] for x in runs), 3)
    out["adaptive_denoise_again_ms"] = round(min(x[1] for x in runs), 3)
    raw, plain = runs[0][2], runs[0][3]
    if not a.plain_only:
        bake_first = session(r, a.spp, True)[0]            # this context's first demodulating call: it bakes the table
        runs = [session(r, a.spp, True) for _ in range(a.repeat)]
        first = min(x[0] for x in runs)
        out["adaptive_denoise_albedo_ms"] = round(first, 3)
        out["adaptive_denoise_albedo_again_ms"] = round(min(x[1] for x in runs), 3)
        out["albedo_bake_1024_ms"] = round(bake_first - first, 3)
        out["albedo_vs_plain"] = round(first / out["adaptive_denoise_ms"], 4)
        out["albedo_vs_plain_again"] = round(out["adaptive_denoise_albedo_again_ms"] / out["adaptive_denoise_again_ms"], 4)
        demod = runs[0][3]
    if a.time_only:
        print(json.dumps(out))
        return
    film = torch.zeros((W * H, 4), dtype=torch.float32, device="cuda")
    r.render_pass_device(0, a.truth_spp, film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    truth = film.cpu().numpy().astype(np.float64)
    truth = truth[:, :3] / truth[:, 3:4]

    def mse(f):
        return float(np.mean((f[:, :3].astype(np.float64) / np.maximum(f[:, 3:4], 1) - truth) ** 2))
    out.update(truth_spp=a.truth_spp, mse_unfiltered=mse(raw), mse_filtered=mse(plain), mse_demodulated=mse(demod))
    line = json.dumps(out)
    Path(a.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
