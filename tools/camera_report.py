#!/usr/bin/env python3
"""The camera sample held to its float64 statement -> profiles/camera_reference.json (DESIGN.md §5 "Camera sample").

usage: tools/camera_report.py [--gpu] [--out profiles/camera_reference.json]

Per case of tests/camera_reference.py (cameras, filters, jitter, independent, Sobol): the derived float32 allowance
(the rounding counts k and what they come to in the case's units) and the worst deviation the oracle reaches; with
--gpu (needs an MI355X) also the worst deviation of k_generate through rt_debug_samples.  The hold_* statements assert
while they measure: a case that fails stops the report.  Without --gpu an existing file's "gpu" entries are kept."""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--gpu", action="store_true")
    p.add_argument("--out", default=str(ROOT / "profiles" / "camera_reference.json"))
    a = p.parse_args()
    import camera_reference as cr
    from computational_ray_tracer_amd import capi
    from oracle import oracle

    oracle.build()
    sources = {"oracle": oracle.OracleScene}
    if a.gpu:
        from computational_ray_tracer_amd.renderer import Renderer
        sources["gpu"] = Renderer
    cases = {}
    for name in cr.cameras():
        cases["camera/" + name] = lambda s, n=name: cr.hold_camera_case(s, n)
    for name in cr.FILTERS:
        cases["filter/" + name] = lambda s, n=name: cr.hold_filter_case(s, n)
    for name in ("triangle", "lanczos"):
        cases[f"filter/{name}/3x3"] = lambda s, n=name: cr.hold_filter_case(s, n, 3)
    cases["jitter"] = cr.hold_jitter_case
    for name in (None, "gaussian"):
        cases[f"independent/{name or 'box'}"] = lambda s, n=name: cr.hold_independent_case(s, n)
    for res in ((12, 8), (12, 10)):
        for r in range(4):
            cases[f"sobol/{res[0]}x{res[1]}/randomize{r}"] = lambda s, r=r, res=res: cr.hold_sobol_case(s, r, res)
    out_path = Path(a.out)
    old = json.loads(out_path.read_text()) if out_path.exists() else {}
    out = {"u": cr.U, "k": cr.allowance(cr.cameras()["perspective"])["k"], "ks_bound": cr.ks_bound(6144), "cases": {}}
    if a.gpu:
        out["library"] = capi.library_sha16()
    elif "library" in old:
        out["library"] = old["library"]
    for cname, fn in cases.items():
        entry = {}
        kind, sub = cname.split("/")[:2] if "/" in cname else (cname, "")
        if kind in ("camera", "filter"):
            cam = cr.cameras()[sub if kind == "camera" else "perspective"]
            f, radius, param = cr.FILTERS[sub] if kind == "filter" else (cr.BOX, (0.5, 0.5), 0.0)
            al = cr.allowance(cam, f, radius, param)
            entry["allowance"] = {"raster": list(al["raster"]), "u": list(al["u"]), "origin": al["origin"],
                                  "norm": al["norm"], "table": [cr.table_bound(f, r, param) for r in radius]}
        for sname, src in sources.items():
            entry[sname] = fn(src)
        if "gpu" not in entry and "gpu" in old.get("cases", {}).get(cname, {}):
            entry["gpu"] = old["cases"][cname]["gpu"]
        out["cases"][cname] = entry
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
