"""Register counts of the four packed single-leaf (Cornell) kernels, read from the built library's code-object metadata
(DESIGN.md §4): rt_kernels.hip is compiled without the SLP vectoriser, which took the bounce-depth shade and the depth-0
trace under the 96-VGPR line (5 waves per SIMD on gfx950: 512 VGPRs per lane, allocated in blocks of 8) and lowered the
other two.  The library's .hip_fatbin section is a row of offload bundles, one per translation unit; each is cut out,
unbundled with clang-offload-bundler and its AMDGPU metadata note printed with llvm-readelf.  No GPU needed.

.private_segment_fixed_size is not asserted on: it reports 36 B for both packed shade instantiations although no
scratch instruction is behind it (SGPR spill slots that end up in VGPR lanes)."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from computational_ray_tracer_amd import capi

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NS = "_ZN4rtmi"
# mangled-name prefix -> (VGPRs with the SLP vectoriser on, i.e. before the flag; the bound this build must meet)
KERNELS = {
    NS + "12k_path_shadeILi1ELb1ELb1EEE": (118, 96),        # k_path_shade<1, true, true>: bounce depths
    NS + "12k_path_shadeILi1ELb0ELb1EEE": (120, 120),       # k_path_shade<1, false, true>: depth 0
    NS + "15k_trace_closestILi1ELb0ELb1ELb1EEE": (108, 108),  # k_trace_closest<1, false, true, true>: bounce depths
    NS + "15k_trace_closestILi1ELb0ELb0ELb1EEE": (109, 96),   # k_trace_closest<1, false, false, true>: depth 0
}


def llvm_tool(name):
    roots = [os.environ.get("ROCM_PATH"), os.environ.get("ROCM_HOME"), "/opt/rocm"]
    for r in filter(None, roots):
        for sub in ("lib/llvm/bin", "llvm/bin"):
            p = Path(r) / sub / name
            if p.exists():
                return str(p)
    return shutil.which(name)


@pytest.fixture(scope="module")
def vgprs(tmp_path_factory):
    """{mangled kernel name: .vgpr_count} over every gfx950 code object of the built library."""
    bundler, readelf = llvm_tool("clang-offload-bundler"), llvm_tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf not found")
    lib = capi.library_path()
    assert lib.exists(), f"{lib} is missing: build first"
    data = lib.read_bytes()
    offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    assert offs, "no offload bundle in the library"
    tmp = tmp_path_factory.mktemp("kres")
    out = {}
    for i, o in enumerate(offs):
        chunk, co = tmp / f"bundle{i}", tmp / f"bundle{i}.co"
        chunk.write_bytes(data[o:offs[i + 1] if i + 1 < len(offs) else len(data)])
        subprocess.run([bundler, "--unbundle", "--type=bc", f"--input={chunk}", f"--targets={TARGET}",
                        f"--output={co}"], check=True, capture_output=True)
        notes = subprocess.run([readelf, "--notes", str(co)], check=True, capture_output=True, text=True).stdout
        name = None
        for line in notes.splitlines():  # (a kernel's keys are sorted: .name comes before .vgpr_count)
            m = re.match(r"\s+(?:- )?\.(name|vgpr_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                name = m.group(2)
            elif name and name.startswith("_Z"):
                out[name] = int(m.group(2))
                name = None
    return out


@pytest.mark.parametrize("prefix", sorted(KERNELS))
def test_packed_cornell_kernels_vgprs(vgprs, prefix):
    names = [n for n in vgprs if n.startswith(prefix)]
    assert len(names) == 1, f"{prefix}: {names}"
    before, bound = KERNELS[prefix]
    v = vgprs[names[0]]
    print(f"{names[0][:60]}: {v} VGPRs (before {before}, bound {bound})")
    assert v <= before and v <= bound
