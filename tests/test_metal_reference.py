"""CPU: the metals' host functions (rt_metal_nk, rt_fresnel_conductor) bit for bit against part 1 of
tests/metal_reference.py, part 1 against the float64 part 2 within twice its measured error, pinned values, six sabotaged
variants that must each fail a named assertion, and rt_fresnel.h with the host table construction under
AddressSanitizer and UBSan in a program of its own.

The named assertions and the six sabotage tests act on the reference's own functions (as tests/test_rough_reference.py's
do): they show that the reference can tell these mistakes.  The library is tied to the reference by the bit tests above
them and by tests/test_gpu_metal.py, not by them."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import metal_reference as mr
import radiometry_reference as ref
import rough_reference as rr
from computational_ray_tracer_amd import scene

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32
NCOS = 2500


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def reference_inputs():
    """Per metal: every table entry (471) x NCOS cosines from 0 to 1, both ends included."""
    c = np.linspace(0.0, 1.0, NCOS).astype(f32)
    assert c[0] == 0 and c[-1] == 1
    return c


def rounding_wavelengths():
    edge = np.array([359.4, 359.5, 830.49, 830.5, 830.51, 359.49], f32)
    halves = (np.arange(359, 831) + 0.5).astype(f32)
    rng = np.random.default_rng(11)
    return np.concatenate([edge, halves, np.nextafter(halves, f32(0)), (355 + 480 * rng.random(10000)).astype(f32)])


# ------------------------------------------------------------------------------------------ bit tests

@pytest.mark.parametrize("metal", mr.METALS)
def test_metal_nk_bit_for_bit(metal):
    lam = rounding_wavelengths()
    assert len(lam) > 10 ** 4
    n, k = scene.metal_nk(metal, lam)
    wn, wk = mr.metal_nk32(metal, lam)
    assert np.array_equal(bits(n), bits(wn)) and np.array_equal(bits(k), bits(wk))
    # the edges: 359.4 rounds to 359 (outside), 359.5 to 360, 830.49 to 830, 830.5 to 831 (outside)
    assert n[0] == 0 and k[0] == 0 and n[3] == 0 and k[3] == 0
    tn, tk = mr.nk32(metal)
    assert n[1] == tn[0] and k[1] == tk[0] and n[2] == tn[470] and k[2] == tk[470]
    # every table entry
    n, k = scene.metal_nk(metal, np.arange(360, 831, dtype=f32))
    assert np.array_equal(bits(n), bits(tn)) and np.array_equal(bits(k), bits(tk))


@pytest.mark.parametrize("metal", mr.METALS)
def test_fresnel_bit_for_bit(metal):
    c = reference_inputs()
    tn, tk = mr.nk32(metal)
    rng = np.random.default_rng(3)
    j = rng.integers(0, mr.NSPEC, 4 * NCOS)
    cc = np.tile(c, 4)
    assert len(cc) == 10 ** 4
    got = scene.fresnel_conductor(cc, tn[j], tk[j])
    assert np.array_equal(bits(got), bits(mr.fresnel32(cc, tn[j], tk[j])))
    # every entry at both ends and in the middle; cosines outside [0, 1] are clamped
    for cv in (0.0, 1.0, 0.3, -0.5, 1.5):
        got = scene.fresnel_conductor(np.full(mr.NSPEC, cv, f32), tn, tk)
        assert np.array_equal(bits(got), bits(mr.fresnel32(np.full(mr.NSPEC, cv, f32), tn, tk))), cv
    assert np.array_equal(bits(scene.fresnel_conductor(np.full(mr.NSPEC, 1.5, f32), tn, tk)),
                          bits(scene.fresnel_conductor(np.ones(mr.NSPEC, f32), tn, tk)))


# ------------------------------------------------------------------------------------------ float64 bound

def _errors():
    c = reference_inputs()
    eF = enk = 0.0
    for metal in mr.METALS:
        tn, tk = mr.nk32(metal)
        n64, k64 = mr.nk64(metal)
        enk = max(enk, np.max(np.abs(tn / n64 - 1)), np.max(np.abs(tk / k64 - 1)))
        got = mr.fresnel32(c[:, None], tn[None, :], tk[None, :]).astype(np.float64)
        eF = max(eF, np.max(np.abs(got - mr.F64(c[:, None].astype(np.float64), n64[None, :], k64[None, :]))))
    return dict(F=float(eF), nk=float(enk))


def test_float32_restatement_within_twice_its_measured_error():
    e = _errors()
    print(f"\nmeasured: {e}")
    b = mr.bounds()
    assert e["F"] <= b["F"] and e["nk"] <= b["nk"], (e, b)
    # MEASURED is what this run measures, to the two digits written down
    assert e["F"] >= 0.5 * mr.MEASURED["F"] and e["nk"] >= 0.5 * mr.MEASURED["nk"], (e, mr.MEASURED)


def test_real_form_equals_the_complex_form_in_float64():
    """The formula of rt_fresnel.h evaluated in float64 agrees with 1/2 (|r_s|^2 + |r_p|^2) to 1e-14 on the four tables."""
    c = np.linspace(0, 1, 501)[:, None]
    for metal in mr.METALS:
        n, k = (a[None, :] for a in mr.nk64(metal))
        c2 = c * c
        s2 = 1 - c2
        t0 = (n * n - k * k) - s2
        ab = np.sqrt(t0 * t0 + 4 * n * n * k * k)
        a = np.sqrt(np.maximum(0.5 * (ab + t0), 0))
        t1, t2 = ab + c2, 2 * a * c
        Rs = (t1 - t2) / (t1 + t2)
        t3, t4 = c2 * ab + s2 * s2, t2 * s2
        F = 0.5 * (Rs * (t3 - t4) / (t3 + t4) + Rs)
        assert np.max(np.abs(F - mr.F64(c, n, k))) < 1e-14


# ------------------------------------------------------------------------------------------ named assertions

PINNED = {("Au", 450): 0.386, ("Au", 550): 0.848, ("Au", 650): 0.940, ("Cu", 450): 0.553, ("Cu", 550): 0.634,
          ("Cu", 650): 0.941, ("Ag", 550): 0.960, ("Al", 550): 0.921}


def assert_pinned_normal_incidence(nk_of, fresnel):
    """F(1) of the four tables at known wavelengths, to the three digits of the issue."""
    for (metal, lam), want in PINNED.items():
        n, k = nk_of(metal)
        got = float(fresnel(1.0, n[lam - 360], k[lam - 360]))
        assert abs(got - want) < 6e-4, (metal, lam, got, want)


def assert_angle_dependence(fresnel):
    """F against the complex form over the angle for every table entry; F -> 1 as cos -> 0; gold at 450 nm rises by 1.27
    from head-on to cos 0.3."""
    c = np.linspace(0, 1, 201)[:, None]
    for metal in mr.METALS:
        n, k = (a[None, :] for a in mr.nk64(metal))
        assert np.max(np.abs(fresnel(c, n, k) - mr.F64(c, n, k))) < 1e-3, metal
        assert np.all(np.abs(fresnel(np.zeros((1, 1)), n, k) - 1) < 1e-6), metal
    n, k = mr.nk64("Au")
    assert abs(float(fresnel(0.3, n[90], k[90]) / fresnel(1.0, n[90], k[90])) - 1.27) < 0.005


def assert_half_vector_argument(cos_of, tol=1e-12):
    """The Fresnel cosine is wo.h: 1 for wi = wo however low wo is, cos of half the angle between a symmetric pair."""
    for muo in (0.05, 0.3, 0.9):
        wo = rr.wo_of(muo)
        assert abs(float(cos_of(wo, wo)) - 1) < tol, muo
        wi = wo * np.array([-1.0, 1.0, 1.0])
        assert abs(float(cos_of(wo, wi)) - muo) < tol, muo
    wo, wi = rr.wo_of(0.9), rr.nrm64(np.array([0.2, 0.6, 0.3]))
    assert abs(float(cos_of(wo, wi)) - math_cos_half(wo, wi)) < tol


def math_cos_half(wo, wi):
    return float(np.sqrt(0.5 * (1 + wo @ wi)))


def assert_rounded_index(index_of):
    """The table is read at the rounded wavelength: x.5 goes up, just below x.5 goes down."""
    lam = np.array([449.5, 449.49, 450.49, 450.5, 360.0, 830.0], f32)
    assert list(index_of(lam)) == [90, 89, 90, 91, 0, 470]


def assert_dielectric_limit(fresnel):
    """k = 0 is fr_dielectric in float64."""
    for eta in (1.33, 1.5168, 2.4):
        for c in (1.0, 0.7, 0.2):
            assert abs(float(fresnel(c, eta, 0.0)) - float(ref.fr_dielectric(c, eta))) < 1e-12, (eta, c)


def test_reference_passes_its_named_assertions():
    assert_pinned_normal_incidence(mr.nk64, mr.F64)
    assert_pinned_normal_incidence(lambda m: tuple(a.astype(np.float64) for a in mr.nk32(m)), mr.F64)
    assert_pinned_normal_incidence(mr.nk32, lambda c, n, k: mr.fresnel32(f32(c), n, k))
    assert_angle_dependence(mr.F64)
    assert_half_vector_argument(mr.cos_h64)
    assert_half_vector_argument(lambda a, b: mr.cos_h32(a.astype(f32), b.astype(f32)), tol=1e-6)
    assert_rounded_index(mr.index32)
    assert_dielectric_limit(mr.F64)


def test_sabotaged_n_and_k_swapped():
    with pytest.raises(AssertionError):
        assert_pinned_normal_incidence(lambda m: mr.nk64(m)[::-1], mr.F64)


def test_sabotaged_gold_table_for_copper():
    with pytest.raises(AssertionError):
        assert_pinned_normal_incidence(lambda m: mr.nk64("Au" if m == "Cu" else m), mr.F64)


def test_sabotaged_schlick_from_normal_incidence():
    with pytest.raises(AssertionError):
        assert_angle_dependence(mr.schlick64)


def test_sabotaged_fresnel_of_normal_incidence_at_every_angle():
    with pytest.raises(AssertionError):
        assert_angle_dependence(lambda c, n, k: mr.F64(1.0, n, k) + 0 * c)


def test_sabotaged_fresnel_at_mu_o():
    with pytest.raises(AssertionError):
        assert_half_vector_argument(lambda wo, wi: wo[2])


def test_sabotaged_table_read_at_the_floor_wavelength():
    with pytest.raises(AssertionError):
        assert_rounded_index(lambda lam: mr.index32(lam, floor=True))


def test_grazing_case_tells_the_angle_dependence():
    """M1g's precondition, in float64 on the CPU: with F(lambda, 1) at every angle, or Schlick from F(1), the Z channel's
    frame mean moves by more than twice its tolerance; and wo.h stays at or below 0.35 on the included pixels."""
    cfg, mu, vmax, include = mr.m1_distant("Au", 0.5, graze=True)
    fc, ch, _ = mr._floor_terms(cfg, 0.5, mr.GRAZE_DIR, ref._midpoints())
    assert ch[include].max() <= 0.35
    tol = ref.tolerance(mu[include], vmax, 256)
    for name, fr in (("F(1)", lambda c, n, k: mr.F64(1.0, n, k) + 0 * c), ("Schlick", mr.schlick64)):
        other = mr.m1_distant("Au", 0.5, graze=True, fresnel=fr)[1]
        shift = abs(other[include, 2].mean() - mu[include, 2].mean())
        print(f"\n{name}: Z mean moves by {shift / tol[2]:.1f} tolerances")
        assert shift > 2 * tol[2], name


# ------------------------------------------------------------------------------------------ sanitizers

SANITIZED = r"""
#include <cstdio>
#include <vector>
#include "rt_fresnel.h"
#include "../data/spectra_data.h"
using namespace rtmi;
int main() {
    const float* eta[4] = {rtdata::metal_ag_eta, rtdata::metal_al_eta, rtdata::metal_au_eta, rtdata::metal_cu_eta};
    const float* kk[4] = {rtdata::metal_ag_k, rtdata::metal_al_k, rtdata::metal_au_k, rtdata::metal_cu_k};
    const int en[4] = {rtdata::metal_ag_eta_n, rtdata::metal_al_eta_n, rtdata::metal_au_eta_n, rtdata::metal_cu_eta_n};
    const int kn[4] = {rtdata::metal_ag_k_n, rtdata::metal_al_k_n, rtdata::metal_au_k_n, rtdata::metal_cu_k_n};
    double sum = 0;
    for (int m = 0; m < kMetals; ++m) {
        std::vector<float> nk(2 * kMetalSpecN);          // (heap: an overrun is a report)
        metal_nk_build(eta[m], en[m], kk[m], kn[m], nk.data());
        for (int j = 0; j < kMetalSpecN; ++j)
            for (int i = 0; i <= 64; ++i) sum += fresnel_conductor(i / 64.0f, nk[2 * j], nk[2 * j + 1]);
        // the ends of the measured tables and beyond them
        const float lam[6] = {eta[m][0], eta[m][en[m] - 2], 200.f, 900.f, 360.f, 830.f};
        for (float l : lam) sum += metal_table_query(eta[m], en[m], l) + metal_table_query(kk[m], kn[m], l);
        sum += (double)metal_index(359.5f) + (double)metal_index(830.49f);
    }
    sum += fresnel_conductor(-1.f, 0.f, 0.f) + fresnel_conductor(2.f, 1.5f, 0.f);
    std::printf("%.6f\n", sum);
    return 0;
}
"""


def test_fresnel_header_and_table_construction_under_sanitizers(tmp_path):
    src = tmp_path / "metal_san.cpp"
    src.write_text(SANITIZED)
    exe = tmp_path / "metal_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                        "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    # (run as tests/test_pass_plan.py runs its sanitized program: the inherited environment without the RTMI_* knobs)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    assert float(out.stdout) > 0
