"""GPU: k_generate's camera sample (camera_sample() in rt_kernels.hip: sampler -> filter offset -> raster position ->
camera model -> world ray) held to the float64 statement of tests/camera_reference.py, through rt_debug_samples.

Scene: the frequency-3 blob of cfg0_reference (180 triangles, reference integrator), a 12 x 8 film (12 x 10 as well
for Sobol), every pixel times every sample index: at most 24 576 records per case.  Every case has a rotated look
(0.3, -0.2, 1), the eye at (27, -13, -80) and a non-square film, the filter cases rx != ry, so that transposes and x/y
swaps cannot cancel.

The statements themselves (camera_reference.hold_*) are the ones tests/test_camera_reference.py runs on the oracle:
no draw is predicted; the returned rays are inverted in float64 to raster positions, lens points and draws, and each
pixel's set of draws must be the stratum grid, each cell exactly once.  Every pixel and every index is asserted.

Tolerances (camera_reference's module docstring): a count of the float32 roundings between the draw and the record
— RASTER_K = 8 on (res + 1) u, DIR_K = 40 u on a direction component, ORG_K = 9 on |o_cam|_1 + |eye|, LENS_K = 16 on
the lens radius, u = 2^-24 — mapped to raster units per camera, asserted below 1/100 of a stratum in every case; for
the tabulated filters 2 h max pdf in CDF space on top (4.9e-4 / 3.7e-4 Gaussian, 1.75e-3 / 1.39e-3 Lanczos), below a
quarter of a stratum.  profiles/camera_reference.json (tools/camera_report.py) lists what each case comes to and the
worst deviation the oracle and the GPU reach."""
import pytest

import camera_reference as cr
from computational_ray_tracer_amd import capi
from computational_ray_tracer_amd.renderer import Renderer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["perspective", "perspective_lens", "perspective_aspect_fix", "orthographic",
                                  "pinhole", "thinlens"])
def test_camera_rays_are_the_stratum_grid(name):
    """Cameras x StratifiedSampler(4, 4, False), box filter 0.5: per pixel the recovered pixel draws are the 4 x 4
    grid and the lens points the mapped grid, each once; lens-free perspective origins are the eye exactly; lens and
    sensor origins lie in their plane; |rd| = 1; weight 1."""
    cr.hold_camera_case(Renderer, name)


@pytest.mark.parametrize("name,n", [(k, 16) for k in cr.FILTERS] + [("triangle", 3), ("lanczos", 3)])
def test_camera_filter_offsets_invert_to_the_grid(name, n):
    """Filters x StratifiedSampler(n, n, False): the exact CDF of the recovered offsets is the n x n grid per pixel.
    (3 x 3: a grid that u -> u + 1/2 does not map onto itself, for the halves of the tent and of a table.)"""
    cr.hold_filter_case(Renderer, name, n)


def test_camera_jittered_strata():
    """StratifiedSampler(4, 4, True), perspective camera with a lens: floor(4 u) of the pixel draws and of the lens
    draws covers the 16 cells once per pixel; the offsets are not at the centres."""
    cr.hold_jitter_case(Renderer)


@pytest.mark.parametrize("name", [None, "gaussian"])
def test_camera_independent_sampler_is_uniform(name):
    """IndependentSampler(64): Kolmogorov-Smirnov on the pooled recovered draws per axis (n = 6144), D < sqrt(ln(2 /
    1e-6) / 2n) = 0.034 (+ the table bound for the Gaussian); the seed is fixed, so this is deterministic."""
    cr.hold_independent_case(Renderer, name)


@pytest.mark.parametrize("res", [(12, 8), (12, 10)])
@pytest.mark.parametrize("randomize", [capi.RT_SOBOL_NONE, capi.RT_SOBOL_PERMUTE_DIGITS, capi.RT_SOBOL_FAST_OWEN,
                                       capi.RT_SOBOL_OWEN])
def test_camera_sobol_pixel_samples(randomize, res):
    """SobolSampler(16), scale 16: every sample lands in its own pixel (edge pixels included) and the 16 offsets of
    every pixel hold one point in every elementary interval 16x1, 8x2, 4x4, 2x8, 1x16."""
    cr.hold_sobol_case(Renderer, randomize, res)
