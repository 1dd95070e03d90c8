"""CPU: rough glass (RT_MAT_ROUGH_DIELECTRIC).  The library's host functions rt_roughglass_eval /
rt_roughglass_sample against the numpy float32 restatement bit for bit, that restatement against float64, the float64
statements' own properties (the bounce weights' means against the two directional albedos by quadrature, energy,
reciprocity, the limits er -> 1 and total internal reflection), which eight sabotaged variants must break, and the
header under the sanitizers in a program of its own.
"""
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rough_reference as rr
import roughglass_reference as rg
from computational_ray_tracer_amd import capi, scene

ROOT = Path(__file__).resolve().parents[1]
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"
f32 = np.float32
N_PER = 400          # x 5 alphas x 5 relative indices = 10^4 inputs
ONE_M = np.nextafter(f32(1), f32(0))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def reference_inputs(alpha, er, n=N_PER, seed=11):
    """(wo, wi, disk, u) float32: local unit wo from grazing (mu_o = 1e-3) to the normal, both T1 branches of the
    sampling among them (wo at and next to the normal); wi over the upper hemisphere, near the lobe, and a few below;
    disk points in the disk, on its rim and at its centre; u over [0, 1) with 0 and nextafter(1, 0).  For er < 1 the
    grazing half of the set lies beyond the critical angle."""
    rng = np.random.default_rng(seed + int(round(alpha * 1000)) + int(round(er * 77)))
    mu = np.concatenate([np.full(n // 40, 1e-3), np.geomspace(1e-3, 1.0, n // 8), rng.random(n - n // 40 - n // 8 - 20),
                         np.full(14, 1.0), 1.0 - np.geomspace(1e-9, 5e-6, 3), 1.0 - np.geomspace(2e-5, 1e-3, 3)])
    phi = rng.random(n) * 2 * math.pi
    st = np.sqrt(np.maximum(0.0, 1 - mu * mu))
    wo = np.stack([st * np.cos(phi), st * np.sin(phi), mu], -1).astype(f32)
    wi = rr.nrm64(rng.normal(size=(n, 3)))
    wi[: n - 20, 2] = np.abs(wi[: n - 20, 2])                         # (the last 20 keep their sign: some lie below)
    wi[:60] = rr.nrm64(wo[:60].astype(np.float64) * [-1, -1, 1] + 0.3 * alpha * rng.normal(size=(60, 3)))
    r, t = np.sqrt(rng.random(n)), rng.random(n) * 2 * math.pi
    r[:3] = 1.0
    r[30:40] = 0.0
    disk = np.stack([r * np.cos(t), r * np.sin(t)], -1).astype(f32)
    k = np.maximum(f32(1), np.sqrt(disk[:, 0] * disk[:, 0] + disk[:, 1] * disk[:, 1]))
    disk = (disk / k[:, None]).astype(f32)
    disk[40:44] = [[1, 0], [-1, 0], [0, 1], [0, -1]]
    u = rng.random(n).astype(f32)
    u[50::194] = 0.0                                                  # (indices past the rim and centre points: a rim point's
    u[55::194] = ONE_M                                                # h is ill-conditioned in float32, pz = sqrt(0 +- eps))
    u = np.minimum(u, ONE_M)
    perm = rng.permutation(n)                                         # (the special u and disk points meet every kind of wo)
    return wo, wi.astype(f32), disk[perm], u[perm]


def _all_inputs():
    for a in rg.ALPHAS:
        for er in rg.ETAS:
            yield (a, er) + reference_inputs(a, er)


def test_library_equals_the_restatement_bit_for_bit():
    total, branches = 0, np.zeros(3, int)
    for a, er, wo, wi, disk, u in _all_inputs():
        fc, pdf = scene.roughglass_eval(a, er, wo, wi)
        fc2, pdf2 = rg.eval32(a, er, wo, wi)
        assert np.array_equal(bits(fc), bits(fc2)) and np.array_equal(bits(pdf), bits(pdf2)), (a, er)
        w, wt, sp, br = scene.roughglass_sample(a, er, wo, disk, u)
        w2, wt2, sp2, br2 = rg.sample32(a, er, wo, disk, u)
        assert np.array_equal(br, br2), (a, er, int(np.sum(br != br2)))
        assert np.array_equal(bits(w), bits(w2)) and np.array_equal(bits(wt), bits(wt2)), (a, er)
        assert np.array_equal(bits(sp), bits(sp2)), (a, er)
        assert np.all(np.isfinite(fc)) and np.all(np.isfinite(pdf)) and np.all(np.isfinite(wt)) and np.all(np.isfinite(sp))
        assert np.all(w[br == 1][:, 2] > 0) and np.all(w[br == 2][:, 2] < 0) and np.all(sp[br != 1] == 0)
        assert np.all(wt[br == 1] <= f32(1.0000005)) and np.all(wt[br == 2] <= f32(1.0000005) / f32(er * er))
        # the eval is F times rt_ggx_eval's values, and 0 below
        g_fc, g_pdf = scene.ggx_eval(a, wo, wi)
        assert np.all(fc <= g_fc) and np.all(pdf <= g_pdf) and np.all(fc[wi[:, 2] <= 0] == 0)
        if er < 1:                                                    # inputs beyond the critical angle
            deep = wo[:, 2] < 0.5 * math.sqrt(1 - er * er)
            assert deep.sum() > 50
        branches += np.bincount(br, minlength=3)
        total += len(wo)
    assert total == 10 ** 4 and np.all(branches > 500), branches


def _rel(got, want, tiny=1e-30):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    big = np.abs(want) >= tiny
    assert np.all(np.abs(got - want)[~big] <= tiny)
    return float(np.max(np.abs(got - want)[big] / np.abs(want)[big])) if big.any() else 0.0


def test_float32_restatement_against_float64():
    worst = dict(fcos=0.0, pdf=0.0, w=0.0, spdf=0.0, wi=0.0)
    n_fragile = n_all = 0
    for a, er, wo, wi, disk, u in _all_inputs():
        wo64, wi64 = rr.nrm64(wo.astype(np.float64)), rr.nrm64(wi.astype(np.float64))
        er64 = float(f32(er))
        fc, pdf = rg.eval32(a, er, wo, wi)
        worst["fcos"] = max(worst["fcos"], _rel(fc, rg.fr_cos64(a, er64, wo64, wi64)))
        worst["pdf"] = max(worst["pdf"], _rel(pdf, rg.pdfF64(a, er64, wo64, wi64)))
        w, wt, sp, br = rg.sample32(a, er, wo, disk, u)
        w64, wt64, sp64, br64, aux = rg.sample64(a, er64, wo64, disk.astype(np.float64), u.astype(np.float64))
        frag = rg.fragile(a, er64, wo64, u.astype(np.float64), aux, disk.astype(np.float64))
        n_fragile += int(frag.sum())
        n_all += len(wo)
        keep = ~frag
        assert np.array_equal(br[keep], br64[keep]), (a, er, int(np.sum(br[keep] != br64[keep])))
        live = keep & (br64 != 0)
        worst["w"] = max(worst["w"], _rel(wt[live], wt64[live]))
        worst["spdf"] = max(worst["spdf"], _rel(sp[live & (br64 == 1)], sp64[live & (br64 == 1)]))
        worst["wi"] = max(worst["wi"], float(np.max(np.abs(w[live].astype(np.float64) - w64[live]))))
    share = n_fragile / n_all
    print(f"fragile share {share:.4f}; measured:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert share <= 0.01, share
    for k, b in rg.bounds().items():
        assert worst[k] <= b, (k, worst[k], b)
        assert worst[k] >= rg.MEASURED[k] / 4, f"{k}: MEASURED is stale ({worst[k]:.3g} against {rg.MEASURED[k]:.3g})"


# ---- properties of the float64 statements, and the sabotaged variants that must break them

@pytest.fixture(scope="module")
def stratified():
    """A 1024^2 stratified disk grid times a stratified u (one stratum per grid point, in a fixed shuffled order)."""
    n = 1024
    g = (np.arange(n) + 0.5) / n
    disk = rr.disk64(np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2))
    u = (np.random.default_rng(1).permutation(n * n) + 0.5) / (n * n)
    return disk, u


PROP_A, PROP_MU = 0.3, 0.5


@pytest.fixture(scope="module")
def albedos():
    return {er: (rg.E_R(PROP_A, PROP_MU, er), rg.E_T(PROP_A, PROP_MU, er)) for er in (1.5, 1 / 1.5)}


def _z(x, want):
    return (x.mean() - want) / (x.std() / math.sqrt(len(x)))


def _weights(stratified, er, a=PROP_A, mu=PROP_MU, **kw):
    """(the reflected weight, the transmitted weight times er^2, 1 / prevPdf over the reflected bounces) per sample."""
    disk, u = stratified
    wi, w, pdf, br, _ = rg.sample64(a, er, rr.wo_of(mu), disk, u, **kw)
    with np.errstate(all="ignore"):
        inv = np.where(br == 1, 1 / pdf, 0.0)
    return np.where(br == 1, w, 0.0), np.where(br == 2, w, 0.0) * er * er, inv


def test_albedos_are_the_recorded_ones(albedos):
    er_, et_ = albedos[1.5]
    assert abs(er_ - 0.0610) < 1e-4 and abs(et_ - 0.8875) < 1e-4, (er_, et_)
    er_, et_ = albedos[1 / 1.5]
    assert abs(er_ - 0.6537) < 1e-4 and abs(et_ - 0.1311) < 1e-4, (er_, et_)


@pytest.mark.parametrize("er", [1.5, 1 / 1.5])
def test_bounce_weights_integrate_to_the_albedos(stratified, albedos, er):
    e_r, e_t = albedos[er]
    wr, wt, inv = _weights(stratified, er)
    zr, zt = _z(wr, e_r), _z(wt, e_t)
    # the library itself on the same grid in float32: its means meet the same quadratures
    disk, u = stratified
    wo32 = np.broadcast_to(rr.wo_of(PROP_MU).astype(f32), (len(disk), 3))
    _, lw, lp, lb = scene.roughglass_sample(PROP_A, er, wo32, disk.astype(f32), np.minimum(u.astype(f32), ONE_M))
    lw = lw.astype(np.float64)
    er32 = float(f32(er))
    lr, lt = np.where(lb == 1, lw, 0.0), np.where(lb == 2, lw, 0.0) * er32 * er32
    print(f"library: reflected mean {lr.mean():.6f} z {_z(lr, e_r):+.2f}; transmitted mean {lt.mean():.6f} z {_z(lt, e_t):+.2f}")
    assert abs(_z(lr, e_r)) < 5, "the library's mean reflected weight equals E_R"
    assert abs(_z(lt, e_t)) < 5, "the library's mean transmitted weight times er^2 equals E_T"
    if er > 1:
        with np.errstate(all="ignore"):
            linv = np.where(lb == 1, 1 / lp.astype(np.float64), 0.0)
        assert abs(_z(linv, 2 * math.pi)) < 5, "the library's prevPdf = F G1 D / (4 mu_o)"
    print(f"er {er:.4f}: E_R {e_r:.6f} mean {wr.mean():.6f} z {zr:+.2f}; E_T {e_t:.6f} mean {wt.mean():.6f} z {zt:+.2f}")
    assert abs(zr) < 5, "the mean reflected weight equals E_R"
    assert abs(zt) < 5, "the mean transmitted weight times er^2 equals E_T"
    assert e_r + e_t <= 1.0, "E_R + E_T <= 1"
    assert e_r + e_t > 0.75                      # (single scattering loses the rest below the two horizons)
    # prevPdf is the density of the reflected directions: E[1 / prevPdf] over them is the upper hemisphere's 2 pi, less
    # the part no visible normal reaches (none at these angles to 1e-3)
    if er > 1:
        assert abs(_z(inv, 2 * math.pi)) < 5, "prevPdf = F G1 D / (4 mu_o)"


def test_reciprocity_of_both_lobes():
    rng = np.random.default_rng(3)
    wo, wi = rr.nrm64(rng.normal(size=(2, 4000, 3)))
    wo[:, 2], wi[:, 2] = np.abs(wo[:, 2]) + 1e-3, np.abs(wi[:, 2]) + 1e-3
    wo, wi = rr.nrm64(wo), rr.nrm64(wi)
    flip = np.array([1.0, 1.0, -1.0])
    for a in (0.2, 0.5, 1.0):
        for er in (1.5, 1 / 1.5, 2.4):
            f1 = rg.fr_cos64(a, er, wo, wi) / wi[:, 2]
            f2 = rg.fr_cos64(a, er, wi, wo) / wo[:, 2]
            assert np.max(np.abs(f1 - f2) / np.maximum(np.abs(f1), 1e-300)) < 1e-10, "reflection lobe reciprocal"
            # f_t(wo, wi) / eta_t^2 = f_t(wi, wo) / eta_i^2: from the other side the frame flips and er inverts
            t1 = rg.ft_cos64(a, er, wo, wi * flip) / wi[:, 2] / (er * er)
            t2 = rg.ft_cos64(a, 1 / er, wi, wo * flip) / wo[:, 2]
            assert (t1 > 0).mean() > 0.2
            # ((wo.ht + er wi.ht)^2 cancels: its relative rounding error is 2^-52 / |wo.ht + er wi.ht|, squared in the
            # lobe, and the half vector's normalisation divides by the same small length; 1e-7 holds 1e-4 of it)
            assert np.max(np.abs(t1 - t2) / np.maximum(np.abs(t1), 1e-300)) < 1e-7, "transmission lobe reciprocal"


def test_limits_unit_index_and_total_internal_reflection(stratified):
    # er -> 1: E_R -> 0 and E_T -> the single-scattering albedo of the interface.  By the bounce's means: next to er = 1
    # F falls from 1 to F(1) within wo.h < 0.01 and the transmission lobe narrows to a point, which no fixed rule resolves
    d8, u8 = stratified[0][::8], stratified[1][::8]
    means = []
    for er1 in (1.5, 1.2, 1.05, 1.0001):
        _, w, _, br, _ = rg.sample64(PROP_A, er1, rr.wo_of(PROP_MU), d8, u8)
        means.append((float(np.where(br == 1, w, 0.0).mean()), float(np.where(br == 2, w, 0.0).mean()) * er1 * er1))
    assert all(a[0] > b[0] for a, b in zip(means[:-1], means[1:])), means
    assert means[-1][0] < 2e-3 and means[-1][1] > 0.9, "er -> 1: E_R -> 0"
    # beyond the critical angle (mu_o = 0.5 < 0.745) at alpha = 0.01: the library's transmitted weight against the share
    # of float64 visible normals that can refract at all (each weight is at most 1 / er^2)
    disk, u = stratified
    disk, u = disk[::64], u[::64]
    er = 1 / 1.5
    _, _, _, _, aux = rg.sample64(0.01, er, rr.wo_of(PROP_MU), disk, u)
    bound = float((aux["s2t"] < 1).mean())
    assert 0 < bound < 0.02                      # (GGX's tails: 0.8 % of the visible normals still refract)
    wo = np.broadcast_to(rr.wo_of(PROP_MU).astype(f32), (len(disk), 3))
    _, w, _, br = scene.roughglass_sample(0.01, er, wo, disk.astype(f32), np.minimum(u.astype(f32), ONE_M))
    e_t = float(np.where(br == 2, w.astype(np.float64), 0.0).mean()) * er * er
    assert e_t <= bound + 1e-6, (e_t, bound)


def test_sabotaged_variants_fail(stratified, albedos):
    e_r, e_t = albedos[1.5]
    b_r, b_t = albedos[1 / 1.5]
    # F at mu_o instead of wo.h: the reflected mean leaves E_R
    assert abs(_z(_weights(stratified, 1.5, f_at_muo=True)[0], e_r)) > 5, "F at mu_o"
    # er not inverted on the back side: the back side's means leave its albedos
    wr, wt, _ = _weights(stratified, 1.5)
    assert abs(_z(wr, b_r)) > 5 and abs(_z(wt * (1 / 1.5) ** 2 / 1.5 ** 2, b_t)) > 5, "er not inverted"
    # the 1 / er^2 missing from the transmitted weight
    assert abs(_z(_weights(stratified, 1.5, no_eta2=True)[1], e_t)) > 5, "1 / er^2 missing"
    # the 1 / er^2 applied to the reflection
    assert abs(_z(_weights(stratified, 1.5, eta2_on_reflection=True)[0], e_r)) > 5, "1 / er^2 on the reflection"
    # a pdf without F: E[1 / prevPdf] leaves 2 pi
    disk, u = stratified
    wi, w, pdf, br, aux = rg.sample64(PROP_A, 1.5, rr.wo_of(PROP_MU), disk, u)
    with np.errstate(all="ignore"):
        inv = np.where(br == 1, aux["F"] / pdf, 0.0)
    assert abs(_z(inv, 2 * math.pi)) > 5, "a pdf without F"
    # Lambda(wt) left out of G2
    assert abs(_z(_weights(stratified, 1.5, no_lambda_wt=True)[1], e_t)) > 5, "Lambda(wt) left out"
    # ht not flipped to the shading side: the lobe's integral leaves the sampled mean
    assert abs(_z(_weights(stratified, 1.5)[1], rg.E_T(PROP_A, PROP_MU, 1.5, rel=1e-6, no_flip=True))) > 5, "ht not flipped"
    # Schlick's polynomial from F(1): no total internal reflection on the back side
    assert abs(_z(_weights(stratified, 1 / 1.5, schlick=True)[0], b_r)) > 5, "Schlick from F(1)"


def test_albedo_tables_between_their_nodes():
    a, er = rg.D3_ALPHA, rg.ETA
    tr, tt = rg.albedo_tables(a, er, 0.96)
    for mu in (0.9712, 1.0):
        # (1e-5: two orders below the float allowance of the films that read the tables; the interpolant's error, measured
        # 1e-6 for E_T at mu_o = 1, not the quadratures')
        assert abs(tr(mu) - rg.E_R(a, mu, er)) < 1e-5 and abs(tt(mu) - rg.E_T(a, mu, er)) < 1e-5, mu


# ---- the header under the sanitizers, in a program of its own

SANITIZED = r"""
#include <cstdio>
#include <vector>
#include "rt_roughglass.h"
using namespace rtmi;
int main() {
    const float alphas[5] = {0.01f, 0.05f, 0.2f, 0.5f, 1.0f};
    const float ers[5] = {1.5f, 1 / 1.5f, 1.0001f, 2.4f, 1 / 2.4f};
    double sum = 0;
    long branches[3] = {0, 0, 0};
    std::vector<float> out(3);                           // (heap: an overrun is a report)
    for (float a : alphas)
        for (float er : ers)
            for (int i = 0; i <= 32; ++i)
                for (int j = 0; j <= 16; ++j) {
                    const float mu = i == 0 ? 1e-3f : i / 32.0f, s = sqrtf(1 - mu * mu);
                    const V3 wo{s, 0.f, mu};
                    const float ph = 0.3926990817f * j, r = j / 16.0f;
                    const float u = j == 0 ? 0.f : j == 16 ? 0.99999994f : j / 16.0f;
                    V3 wi;
                    const int b = roughglass_sample(a, er, wo, r * cosf(ph), r * sinf(ph), u, wi, out[0], out[1]);
                    ++branches[b];
                    sum += out[0] + out[1];
                    float fc, pdf;
                    roughglass_eval(a, er, wo, V3{-s, 0.1f * j, mu}, fc, pdf);
                    sum += fc + pdf;
                    roughglass_eval(a, er, wo, V3{0.f, 0.f, -1.f}, fc, pdf);
                    sum += fc + pdf + roughglass_F(-0.5f + 0.125f * j, er);
                }
    V3 w;
    sum += roughglass_sample(0.5f, 1.5f, V3{0.f, 0.f, -1.f}, 0.f, 0.f, 0.5f, w, out[0], out[1]);
    sum += roughglass_eta_ok(1.5f) + roughglass_eta_ok(0.f) + roughglass_eta_ok(INFINITY);
    std::printf("%.6f %ld %ld %ld\n", sum, branches[0], branches[1], branches[2]);
    return 0;
}
"""


def test_header_under_sanitizers(tmp_path):
    src = tmp_path / "roughglass_san.cpp"
    src.write_text(SANITIZED)
    exe = tmp_path / "roughglass_san"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                        "-I" + HIP_INCLUDE, "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe),
                        str(src)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-4000:]
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]
    vals = out.stdout.split()
    assert math.isfinite(float(vals[0])) and all(int(v) > 0 for v in vals[1:])
