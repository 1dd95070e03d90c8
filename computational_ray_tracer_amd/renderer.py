"""Python host mirror of the reference's render loop (RayTracerTestApp::MainLoop, RayTracerTestApp.h:64-513)
driving the MI355X C-ABI.  `Renderer.render_pass(index_begin, index_end, film)` is the drop-in for one
ThreadFunction/evaluate_pixel dispatch over every pixel (RayTracerTestApp.h:347-422)."""
import ctypes as C

import numpy as np

from . import capi

# rt_denoise_desc defaults (chosen on the oracle's Cornell render, tests/test_denoise_reference.py)
DENOISE_DEFAULTS = dict(iterations=5, feature_samples=4, normal_power_log2=7, sigma_l=1.5, sigma_z=1.0,
                        lum_floor=0.01, depth_floor=0.002)

# rt_temporal_desc defaults (frozen on the oracle's moving-camera Cornell frames,
# tests/test_temporal_reference.py); max_history is 32 frames of 16 samples
TEMPORAL_DEFAULTS = dict(normal_min=0.9, plane_rel=0.01, max_history=512.0, feature_samples=4)

# chain_depth of rt_denoise_desc and rt_temporal_desc: 0 = first-surface guides.  Accepted next to the
# fields above by every call that takes them; kept apart because the two dicts above are pinned to the numpy references'.
CHAIN_DEFAULTS = dict(chain_depth=0)
# chain_curved (same calls): True sets capi.RT_CHAIN_CURVED in the descriptor's chain_depth, the curvature-aware
# virtual distance of DESIGN.md §3e.  Opt-in; kept out of CHAIN_DEFAULTS, which is pinned to the ABI's one field.
CHAIN_CURVED_DEFAULT = False


# albedo_floor of the demodulating filter (rt_denoise_albedo): frozen on the oracle's textured floor at
# 16 spp against the float64 closed form (tests/test_albedo_reference.py), among {1/256, 1/64, 1/16}
ALBEDO_FLOOR_DEFAULT = 1.0 / 256


def chain_arg(chain_depth, chain_curved=CHAIN_CURVED_DEFAULT):
    """The chain_depth value of the C ABI: the depth, with capi.RT_CHAIN_CURVED set when chain_curved."""
    return int(chain_depth) | (capi.RT_CHAIN_CURVED if chain_curved else 0)


class Renderer:
    """One rt_ctx.  `device` is one HIP ordinal or a list of them (rt_options.devices: every pass renders on
    all of them at once, pixel tiles interleaved, the film bit-identical to one device).  Configured from a
    scene.Config (or the individual descriptors)."""

    def __init__(self, cfg=None, device=0, octree_build=capi.RT_OCTREE_BUILD_DEVICE):
        self.lib = capi.load_library()
        opt = capi.rt_options()
        devs = list(device) if isinstance(device, (list, tuple)) else [int(device)]
        if not 1 <= len(devs) <= capi.RT_MAX_DEVICES:
            raise ValueError(f"1..{capi.RT_MAX_DEVICES} devices")
        opt.device = devs[0]
        opt.n_devices = len(devs)
        for i, d in enumerate(devs):
            opt.devices[i] = d
        opt.octree_build = octree_build
        h = C.c_void_p()
        rc = self.lib.rt_create(C.byref(opt), C.byref(h))
        if rc != capi.RT_OK:
            raise capi.RTError("rt_create", rc, "no usable gfx950 device" if rc == capi.RT_E_NODEVICE else "")
        self.h = h
        self.cfg = None
        if cfg is not None:
            self.configure(cfg)

    def _chk(self, name, rc):
        if rc != capi.RT_OK:
            raise capi.RTError(name, rc, self.lib.rt_last_error(self.h).decode())

    def configure(self, cfg):
        self.cfg = cfg
        self._scene = cfg.model.desc()
        self._chk("rt_scene_upload", self.lib.rt_scene_upload(self.h, C.byref(self._scene)))
        tex = cfg.model.texture_desc() if hasattr(cfg.model, "texture_desc") else None
        if tex is not None:  # (the upload dropped any earlier textures)
            self._chk("rt_scene_set_textures", self.lib.rt_scene_set_textures(self.h, C.byref(tex)))
        self._chk("rt_camera_set", self.lib.rt_camera_set(self.h, C.byref(cfg.camera.desc())))
        self._chk("rt_sampler_set", self.lib.rt_sampler_set(self.h, C.byref(cfg.sampler.desc())))
        self._chk("rt_film_set", self.lib.rt_film_set(self.h, C.byref(cfg.film.desc())))
        self._chk("rt_integrator_set", self.lib.rt_integrator_set(self.h, C.byref(cfg.integrator.desc())))
        self.res = cfg.film.res

    # ---- albedo textures (rt_scene_set_textures) -----------------------------------------------
    def set_textures(self, textures, material_texture=None, tri_texcoords=None):
        """Bind scene.Texture images to the uploaded scene's materials: material_texture holds a texture id or -1 per
        material, tri_texcoords (n_triangles, 3, 2) the corners' uv (default: the model's texcoords[indices]).
        textures None or empty clears them.  The reference integrator ignores textures."""
        if not textures:
            self._chk("rt_scene_set_textures", self.lib.rt_scene_set_textures(self.h, None))
            return
        from . import scene
        m = self.cfg.model
        if tri_texcoords is None:
            tri_texcoords = np.asarray(m.texcoords, np.float32)[np.asarray(m.indices, np.int64)]
        d = scene.texture_desc(textures, material_texture, tri_texcoords, max(len(m.materials), 1))
        self._chk("rt_scene_set_textures", self.lib.rt_scene_set_textures(self.h, C.byref(d)))

    def texture_bake(self, rgb8):
        """rt_debug_texture_bake: the bake kernel alone on (..., 3) uint8 texels -> (..., 3) float32 (c0, c1, c2)."""
        a = np.ascontiguousarray(rgb8, np.uint8)
        assert a.ndim >= 1 and a.shape[-1] == 3
        out = np.zeros(a.shape, np.float32)
        self._chk("rt_debug_texture_bake", self.lib.rt_debug_texture_bake(
            self.h, a.size // 3, a.ctypes.data_as(C.POINTER(C.c_uint8)), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def texture_eval(self, prim, b):
        """rt_debug_texture_eval: the shade kernels' texture fetch for triangle ids prim (n) and barycentrics b (n, 3):
        (texel int32 (n): the index within the triangle's texture or -1 when it has none, coeffs float32 (n, 3): the
        (c0, c1, c2) the shade would use)."""
        prim = np.ascontiguousarray(prim, np.int32)
        b = np.ascontiguousarray(b, np.float32)
        assert b.shape == (len(prim), 3)
        texel, co = np.zeros(len(prim), np.int32), np.zeros((len(prim), 3), np.float32)
        self._chk("rt_debug_texture_eval", self.lib.rt_debug_texture_eval(
            self.h, len(prim), prim.ctypes.data_as(C.POINTER(C.c_int32)), b.ctypes.data_as(C.POINTER(C.c_float)),
            texel.ctypes.data_as(C.POINTER(C.c_int32)), co.ctypes.data_as(C.POINTER(C.c_float))))
        return texel, co

    # ---- mesh area lights (capi.RT_LIGHT_MESH) -------------------------------------------------
    def meshlight_table(self, light):
        """rt_debug_meshlight_table: the device table of mesh light `light` -> (tri int32 (n): the light's triangle
        ids, cdf float32 (n), area float32: the total area S_{n-1})."""
        n, area = C.c_int(0), C.c_float(0)
        self._chk("rt_debug_meshlight_table", self.lib.rt_debug_meshlight_table(
            self.h, int(light), C.byref(n), None, None, C.byref(area)))
        tri, cdf = np.zeros(n.value, np.int32), np.zeros(n.value, np.float32)
        self._chk("rt_debug_meshlight_table", self.lib.rt_debug_meshlight_table(
            self.h, int(light), C.byref(n), tri.ctypes.data_as(C.POINTER(C.c_int32)),
            cdf.ctypes.data_as(C.POINTER(C.c_float)), C.byref(area)))
        return tri, cdf, np.float32(area.value)

    def light_sample(self, light, po, u):
        """rt_debug_light_sample: the path kernels' light sampling for shading points po (n, 3) and sample points
        u (n, 2) -> dict(wi (n, 3), tmax (n), dist2 (n), nl (n, 3), tri int32 (n)); tri is -1 unless `light` is a
        mesh light."""
        po = np.ascontiguousarray(po, np.float32)
        u = np.ascontiguousarray(u, np.float32)
        n = len(po)
        assert po.shape == (n, 3) and u.shape == (n, 2)
        wi, nl = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        tmax, dist2, tri = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_light_sample", self.lib.rt_debug_light_sample(
            self.h, int(light), n, po.ctypes.data_as(F), u.ctypes.data_as(F), wi.ctypes.data_as(F),
            tmax.ctypes.data_as(F), dist2.ctypes.data_as(F), nl.ctypes.data_as(F),
            tri.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(wi=wi, tmax=tmax, dist2=dist2, nl=nl, tri=tri)

    # ---- image environment light (rt_scene_set_environment) -------------------------------------
    def set_environment(self, env):
        """Bind a scene.Environment to the uploaded scene as one more light at the end of its list (None clears it;
        configure() drops it).  The path integrators sample it and shade their misses with it; the reference integrator
        and the feature passes ignore it."""
        if env is None:
            self._chk("rt_scene_set_environment", self.lib.rt_scene_set_environment(self.h, None))
            return
        d = env.desc()
        self._chk("rt_scene_set_environment", self.lib.rt_scene_set_environment(self.h, C.byref(d)))

    def env_table(self):
        """rt_debug_env_table: the bound map's device tables -> dict(coeffs (H, W, 4): c0, c1, c2, m; cond (H, W);
        marg (H); total float32)."""
        w, h, tot = C.c_int(0), C.c_int(0), C.c_float(0)
        self._chk("rt_debug_env_table", self.lib.rt_debug_env_table(self.h, C.byref(w), C.byref(h), None, None, None,
                                                                    C.byref(tot)))
        co = np.zeros((h.value, w.value, 4), np.float32)
        cond, marg = np.zeros((h.value, w.value), np.float32), np.zeros(h.value, np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_env_table", self.lib.rt_debug_env_table(
            self.h, C.byref(w), C.byref(h), co.ctypes.data_as(F), cond.ctypes.data_as(F), marg.ctypes.data_as(F),
            C.byref(tot)))
        return dict(coeffs=co, cond=cond, marg=marg, total=np.float32(tot.value))

    def env_sample(self, u):
        """rt_debug_env_sample: the path kernels' environment sampling for sample points u (n, 2) -> dict(wi (n, 3),
        pdf (n): pdf_omega, texel int32 (n): y W + x)."""
        u = np.ascontiguousarray(u, np.float32)
        n = len(u)
        assert u.shape == (n, 2)
        wi, pdf, texel = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_env_sample", self.lib.rt_debug_env_sample(
            self.h, n, u.ctypes.data_as(F), wi.ctypes.data_as(F), pdf.ctypes.data_as(F),
            texel.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(wi=wi, pdf=pdf, texel=texel)

    def env_eval(self, dirs):
        """rt_debug_env_eval: the miss stage's lookup for directions dirs (n, 3) -> dict(texel int32 (n), pdf (n))."""
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(d)
        assert d.shape == (n, 3)
        pdf, texel = np.zeros(n, np.float32), np.zeros(n, np.int32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_env_eval", self.lib.rt_debug_env_eval(
            self.h, n, d.ctypes.data_as(F), texel.ctypes.data_as(C.POINTER(C.c_int32)), pdf.ctypes.data_as(F)))
        return dict(texel=texel, pdf=pdf)

    def env_miss_ms(self):
        """rt_debug_env_stats: the miss stage's HIP-event time (ms) since the last reset_stats()."""
        ms = C.c_double(0)
        self._chk("rt_debug_env_stats", self.lib.rt_debug_env_stats(self.h, C.byref(ms), None))
        return ms.value

    def tabled_launches(self):
        """rt_debug_env_stats' launch counts since the process started: dict(shade=(TL 0, 1, 2), nee=(TL 0, 1, 2)) of
        k_path_shade_full and k_path_nee (debug only: which instantiations a scene runs)."""
        ms, n = C.c_double(0), (C.c_int64 * 6)()
        self._chk("rt_debug_env_stats", self.lib.rt_debug_env_stats(self.h, C.byref(ms), n))
        return dict(shade=np.array(n[0:3], np.int64), nee=np.array(n[3:6], np.int64))

    # ---- rough reflector (capi.RT_MAT_ROUGH) ----------------------------------------------------
    def ggx_sample(self, alpha, normal, dirs, u):
        """rt_debug_ggx_sample: the shade kernel's rough bounce for shading-side normals normal (n, 3), incoming ray
        directions dirs (n, 3) and the bounce's sample points u (n, 2) -> dict(disk (n, 2): the disk point used,
        wi (n, 3): world space, wb (n), pdf (n); all 0 where there is no bounce)."""
        nr = np.ascontiguousarray(normal, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        u = np.ascontiguousarray(u, np.float32)
        n = len(nr)
        assert nr.shape == (n, 3) and d.shape == (n, 3) and u.shape == (n, 2)
        disk, wi = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
        wb, pdf = np.zeros(n, np.float32), np.zeros(n, np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_ggx_sample", self.lib.rt_debug_ggx_sample(
            self.h, float(alpha), n, nr.ctypes.data_as(F), d.ctypes.data_as(F), u.ctypes.data_as(F),
            disk.ctypes.data_as(F), wi.ctypes.data_as(F), wb.ctypes.data_as(F), pdf.ctypes.data_as(F)))
        return dict(disk=disk, wi=wi, wb=wb, pdf=pdf)

    def ggx_eval(self, alpha, normal, dirs, wi):
        """rt_debug_ggx_eval: the shade kernel's rough light term for normals (n, 3), incoming ray directions (n, 3) and
        world-space light directions wi (n, 3) -> dict(fcos (n): f mu_i / R, pdf (n))."""
        nr = np.ascontiguousarray(normal, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        w = np.ascontiguousarray(wi, np.float32)
        n = len(nr)
        assert nr.shape == (n, 3) and d.shape == (n, 3) and w.shape == (n, 3)
        fcos, pdf = np.zeros(n, np.float32), np.zeros(n, np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_ggx_eval", self.lib.rt_debug_ggx_eval(
            self.h, float(alpha), n, nr.ctypes.data_as(F), d.ctypes.data_as(F), w.ctypes.data_as(F),
            fcos.ctypes.data_as(F), pdf.ctypes.data_as(F)))
        return dict(fcos=fcos, pdf=pdf)

    def rough_launches(self):
        """rt_debug_rough_stats: launches of the RGH instantiations of k_path_shade_full and k_path_nee by the last
        path pass, summed (0 for a scene without a rough material)."""
        n = (C.c_int64 * 2)()
        self._chk("rt_debug_rough_stats", self.lib.rt_debug_rough_stats(self.h, n))
        return int(n[0]) + int(n[1])

    # ---- metal (capi.RT_MAT_CONDUCTOR) -----------------------------------------------------------
    def conductor_eval(self, metal, alpha, normal, dirs, wi, lam):
        """rt_debug_conductor_eval: the level-2 kernels' light term at a conductor vertex of metal (an RT_METAL_* id) for
        normals (n, 3), incoming ray directions (n, 3), world-space light directions wi (n, 3) and wavelengths lam (n)
        -> dict(fcos (n), pdf (n): rt_debug_ggx_eval's bits, F (n): F(lambda, wo.h))."""
        nr = np.ascontiguousarray(normal, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        w = np.ascontiguousarray(wi, np.float32)
        lam = np.ascontiguousarray(lam, np.float32)
        n = len(nr)
        assert nr.shape == (n, 3) and d.shape == (n, 3) and w.shape == (n, 3) and lam.shape == (n,)
        fcos, pdf, fr = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_conductor_eval", self.lib.rt_debug_conductor_eval(
            self.h, int(metal), float(alpha), n, nr.ctypes.data_as(F), d.ctypes.data_as(F), w.ctypes.data_as(F),
            lam.ctypes.data_as(F), fcos.ctypes.data_as(F), pdf.ctypes.data_as(F), fr.ctypes.data_as(F)))
        return dict(fcos=fcos, pdf=pdf, F=fr)

    def conductor_launches(self):
        """rt_debug_conductor_stats: launches of the level-2 (rough and conductor) instantiations of k_path_shade_full
        and k_path_nee by the last path pass, summed (0 for a scene without a conductor)."""
        n = (C.c_int64 * 2)()
        self._chk("rt_debug_conductor_stats", self.lib.rt_debug_conductor_stats(self.h, n))
        return int(n[0]) + int(n[1])

    # ---- rough glass (capi.RT_MAT_ROUGH_DIELECTRIC) -----------------------------------------------
    def roughglass_sample(self, alpha, eta_r, normal, dirs, u):
        """rt_debug_roughglass_sample: the level-3 shade kernel's bounce at a rough-glass vertex for shading-side normals
        (n, 3), incoming ray directions (n, 3) and u (n, 3): the bounce's Get2D then the Fresnel choice's Get1D
        -> dict(disk (n, 2), wi (n, 3) world, w (n), pdf (n), branch (n): 0 none, 1 reflected, 2 transmitted)."""
        nr = np.ascontiguousarray(normal, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        u = np.ascontiguousarray(u, np.float32)
        n = len(nr)
        assert nr.shape == (n, 3) and d.shape == (n, 3) and u.shape == (n, 3)
        disk, wi = np.zeros((n, 2), np.float32), np.zeros((n, 3), np.float32)
        w, pdf, br = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.int32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_roughglass_sample", self.lib.rt_debug_roughglass_sample(
            self.h, float(alpha), float(eta_r), n, nr.ctypes.data_as(F), d.ctypes.data_as(F), u.ctypes.data_as(F),
            disk.ctypes.data_as(F), wi.ctypes.data_as(F), w.ctypes.data_as(F), pdf.ctypes.data_as(F),
            br.ctypes.data_as(C.POINTER(C.c_int32))))
        return dict(disk=disk, wi=wi, w=w, pdf=pdf, branch=br)

    def roughglass_eval(self, alpha, eta_r, normal, dirs, wi):
        """rt_debug_roughglass_eval: the level-3 kernels' light term at a rough-glass vertex for normals (n, 3), incoming
        ray directions (n, 3) and world-space light directions wi (n, 3) -> dict(fcos (n), pdf (n)): fcosF, pdfF."""
        nr = np.ascontiguousarray(normal, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        w = np.ascontiguousarray(wi, np.float32)
        n = len(nr)
        assert nr.shape == (n, 3) and d.shape == (n, 3) and w.shape == (n, 3)
        fcos, pdf = np.zeros(n, np.float32), np.zeros(n, np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_roughglass_eval", self.lib.rt_debug_roughglass_eval(
            self.h, float(alpha), float(eta_r), n, nr.ctypes.data_as(F), d.ctypes.data_as(F), w.ctypes.data_as(F),
            fcos.ctypes.data_as(F), pdf.ctypes.data_as(F)))
        return dict(fcos=fcos, pdf=pdf)

    def roughglass_launches(self):
        """rt_debug_roughglass_stats: launches of the level-3 (rough, conductor and rough glass) instantiations of
        k_path_shade_full and k_path_nee by the last path pass, summed (0 for a scene without a rough glass)."""
        n = (C.c_int64 * 2)()
        self._chk("rt_debug_roughglass_stats", self.lib.rt_debug_roughglass_stats(self.h, n))
        return int(n[0]) + int(n[1])

    # ---- absorbing media inside glass (rt_scene_set_media) ---------------------------------------
    def set_media(self, media):
        """Bind one scene.Medium (or None) per material of the uploaded scene; None or an empty list clears them.  Only
        glass materials (RT_MAT_DIELECTRIC, RT_MAT_ROUGH_DIELECTRIC) take sigma > 0."""
        if not media:
            self._chk("rt_scene_set_media", self.lib.rt_scene_set_media(self.h, None, 0))
            return
        from . import scene
        self._chk("rt_scene_set_media", self.lib.rt_scene_set_media(self.h, scene.media_array(list(media)), len(media)))

    def medium_eval(self, media, lam, length):
        """rt_debug_medium_eval: the device function the absorb stage calls, one item per thread: a scene.Medium (or n of
        them), hero wavelengths lam (n, 8), segment lengths (n) -> transmittances (n, 8) float32."""
        from . import scene
        arr, n, lam, length = scene._medium_items(media, lam, length)
        out = np.zeros((n, 8), np.float32)
        F = C.POINTER(C.c_float)
        self._chk("rt_debug_medium_eval", self.lib.rt_debug_medium_eval(
            self.h, arr, n, lam.ctypes.data_as(F), length.ctypes.data_as(F), out.ctypes.data_as(F)))
        return out

    def medium_stats(self):
        """rt_debug_medium_stats: (launches of the absorb stage, segments it attenuated) in the last path pass."""
        n, s = C.c_int(0), C.c_ulonglong(0)
        self._chk("rt_debug_medium_stats", self.lib.rt_debug_medium_stats(self.h, C.byref(n), C.byref(s)))
        return int(n.value), int(s.value)

    def set_shard(self, tile_size, n_shards, shard_id):
        self._chk("rt_set_shard",self.lib.rt_set_shard(self.h, tile_size, n_shards, shard_id))

    def new_film(self):
        return np.zeros((self.res[0] * self.res[1], 4), dtype=np.float32)

    def render_pass(self, index_begin, index_end, film=None):
        """Accumulate sample indices [index_begin, index_end) into `film` (host float32 [W*H, 4])."""
        if film is None:
            film = self.new_film()
        assert film.dtype == np.float32 and film.flags.c_contiguous and film.shape == (self.res[0] * self.res[1], 4)
        self._chk("rt_render_pass", self.lib.rt_render_pass(self.h, index_begin, index_end,
                                                            film.ctypes.data_as(C.POINTER(capi.rt_pixel))))
        return film

    def render_pass_device(self, index_begin, index_end, film_ptr, stream_ptr=None):
        """Accumulate into a device-resident film (e.g. a torch.cuda float32 [W*H, 4] tensor's data_ptr)."""
        self._chk("rt_render_pass_device", self.lib.rt_render_pass_device(
            self.h, index_begin, index_end, C.c_void_p(film_ptr), C.c_void_p(stream_ptr or 0)))

    # ---- adaptive sampling (rt_adaptive_*) ------------------------------------------------------
    @staticmethod
    def _adaptive_desc(min_samples=2, step_samples=1, max_samples=2, rel_error=0.0, abs_floor=1e-3):
        d = capi.rt_adaptive_desc()
        d.min_samples, d.step_samples, d.max_samples = int(min_samples), int(step_samples), int(max_samples)
        d.rel_error, d.abs_floor = float(rel_error), float(abs_floor)
        return d

    @staticmethod
    def _adaptive_info(i):
        return {k: getattr(i, k) for k, _ in i._fields_}

    def n_blocks(self):
        """Image-aligned 8x8 blocks of the film: (columns, rows); block (bx, by) is entry by * columns + bx."""
        return (self.res[0] + 7) // 8, (self.res[1] + 7) // 8

    def render_adaptive(self, min_samples, step_samples, max_samples, rel_error, abs_floor=1e-3):
        """rt_render_adaptive: (film float32 [W*H, 4], moments float32 [W*H, 2] = (sum, sumsq), info dict).  A pixel's
        film.w is the number of indices it took: min_samples, then step_samples more per iteration while its 8x8
        block's error is above rel_error, max_samples at most."""
        d = self._adaptive_desc(min_samples, step_samples, max_samples, rel_error, abs_floor)
        film = self.new_film()
        mom = np.zeros((self.res[0] * self.res[1], 2), np.float32)
        info = capi.rt_adaptive_info()
        self._chk("rt_render_adaptive", self.lib.rt_render_adaptive(
            self.h, C.byref(d), film.ctypes.data_as(C.POINTER(capi.rt_pixel)),
            mom.ctypes.data_as(C.POINTER(capi.rt_moment)), C.byref(info)))
        return film, mom, self._adaptive_info(info)

    def adaptive_begin(self, min_samples, step_samples, max_samples, rel_error, abs_floor=1e-3):
        d = self._adaptive_desc(min_samples, step_samples, max_samples, rel_error, abs_floor)
        self._chk("rt_adaptive_begin", self.lib.rt_adaptive_begin(self.h, C.byref(d)))

    def adaptive_step(self):
        """One iteration; returns the session's rt_adaptive_info as a dict."""
        info = capi.rt_adaptive_info()
        self._chk("rt_adaptive_step", self.lib.rt_adaptive_step(self.h, C.byref(info)))
        return self._adaptive_info(info)

    def adaptive_read(self):
        """The session's state: dict(film, moments, block_error [rows, columns], active = the active pixel ids in
        work-list order)."""
        n = self.res[0] * self.res[1]
        bx, by = self.n_blocks()
        film, mom = self.new_film(), np.zeros((n, 2), np.float32)
        err, act, na = np.zeros((by, bx), np.float32), np.zeros(n, np.int32), C.c_int()
        self._chk("rt_adaptive_read", self.lib.rt_adaptive_read(
            self.h, film.ctypes.data_as(C.POINTER(capi.rt_pixel)), mom.ctypes.data_as(C.POINTER(capi.rt_moment)),
            err.ctypes.data_as(C.POINTER(C.c_float)), act.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(na)))
        return dict(film=film, moments=mom, block_error=err, active=act[: na.value].copy())

    def adaptive_end(self):
        self._chk("rt_adaptive_end", self.lib.rt_adaptive_end(self.h))

    def adaptive_select(self, film, moments, rel_error, abs_floor=1e-3):
        """rt_debug_adaptive_select: the block error estimate and the compaction once, on host arrays, from the full
        list of owned pixels; returns (block_error [rows, columns], active pixel ids)."""
        n = self.res[0] * self.res[1]
        film = np.ascontiguousarray(film, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        assert film.shape == (n, 4) and moments.shape == (n, 2)
        d = self._adaptive_desc(rel_error=rel_error, abs_floor=abs_floor)
        bx, by = self.n_blocks()
        err, act, na = np.zeros((by, bx), np.float32), np.zeros(n, np.int32), C.c_int()
        self._chk("rt_debug_adaptive_select", self.lib.rt_debug_adaptive_select(
            self.h, C.byref(d), film.ctypes.data_as(C.POINTER(capi.rt_pixel)),
            moments.ctypes.data_as(C.POINTER(capi.rt_moment)), err.ctypes.data_as(C.POINTER(C.c_float)),
            act.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(na)))
        return err, act[: na.value].copy()

    # ---- denoiser (rt_render_features, rt_denoise, rt_adaptive_denoise) ------------------------
    @staticmethod
    def _denoise_desc(**kw):
        unknown = set(kw) - set(DENOISE_DEFAULTS) - set(CHAIN_DEFAULTS) - {"chain_curved"}
        if unknown:
            raise TypeError(f"unknown denoise parameters: {sorted(unknown)}")
        p = {**DENOISE_DEFAULTS, **CHAIN_DEFAULTS, **kw}
        d = capi.rt_denoise_desc()
        d.iterations, d.feature_samples = int(p["iterations"]), int(p["feature_samples"])
        d.normal_power_log2 = int(p["normal_power_log2"])
        d.sigma_l, d.sigma_z = float(p["sigma_l"]), float(p["sigma_z"])
        d.lum_floor, d.depth_floor = float(p["lum_floor"]), float(p["depth_floor"])
        d.chain_depth = chain_arg(p["chain_depth"], p.get("chain_curved", CHAIN_CURVED_DEFAULT))
        return d

    def render_features(self, index_begin, index_end, feat=None):
        """Accumulate the first-hit features (normal and depth sums, float32 [W*H, 4]) of sample indices
        [index_begin, index_end) into `feat`."""
        if feat is None:
            feat = self.new_film()
        assert feat.dtype == np.float32 and feat.flags.c_contiguous and feat.shape == (self.res[0] * self.res[1], 4)
        self._chk("rt_render_features", self.lib.rt_render_features(self.h, index_begin, index_end,
                                                                    feat.ctypes.data_as(C.POINTER(capi.rt_feature))))
        return feat

    def render_features_albedo(self, index_begin, index_end, chain_depth=0, feat=None, pos=None, albedo=None,
                               with_pos=True, chain_curved=CHAIN_CURVED_DEFAULT):
        """rt_render_features_albedo: render_features_chain that also accumulates the first-hit albedo film (sensor-RGB
        albedo sums and hit count, float32 [W*H, 4]).  Returns (feat, pos, albedo); with_pos=False:
        (feat, albedo)."""
        feat = self.new_film() if feat is None else feat
        albedo = self.new_film() if albedo is None else albedo
        if with_pos:
            pos = self.new_film() if pos is None else pos
        for a in (feat, pos, albedo) if with_pos else (feat, albedo):
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (self.res[0] * self.res[1], 4)
        self._chk("rt_render_features_albedo", self.lib.rt_render_features_albedo(
            self.h, index_begin, index_end, chain_arg(chain_depth, chain_curved),
            feat.ctypes.data_as(C.POINTER(capi.rt_feature)),
            pos.ctypes.data_as(C.POINTER(capi.rt_position)) if with_pos else None,
            albedo.ctypes.data_as(C.POINTER(capi.rt_albedo))))
        return (feat, pos, albedo) if with_pos else (feat, albedo)

    def albedo_bake(self, coeffs):
        """rt_debug_albedo_bake: the albedo bake kernel alone on (..., 3) float32 sigmoid coefficients -> (..., 3)
        float32 sensor-RGB albedo under the current film's sensor."""
        a = np.ascontiguousarray(coeffs, np.float32)
        assert a.ndim >= 1 and a.shape[-1] == 3
        out = np.zeros(a.shape, np.float32)
        self._chk("rt_debug_albedo_bake", self.lib.rt_debug_albedo_bake(
            self.h, a.size // 3, a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def denoise(self, film, mom, feat, res=None, variance=False, albedo=None, albedo_floor=ALBEDO_FLOOR_DEFAULT,
                **desc):
        """rt_denoise on host arrays of `res` (default: the film's): film [N, 4], moments [N, 2], features [N, 4] of
        desc feature_samples indices -> the filtered film [N, 4] (and the filtered variance [N] with variance=True).
        albedo [N, 4] (render_features_albedo): rt_denoise_albedo, which filters the film divided by the albedo, floored
        at albedo_floor, and multiplies it back.  Descriptor fields default to DENOISE_DEFAULTS."""
        W, H = res or self.res
        film = np.ascontiguousarray(film, np.float32)
        mom = np.ascontiguousarray(mom, np.float32)
        feat = np.ascontiguousarray(feat, np.float32)
        assert film.shape == (W * H, 4) and mom.shape == (W * H, 2) and feat.shape == (W * H, 4)
        d = self._denoise_desc(**desc)
        out = np.zeros((W * H, 4), np.float32)
        var = np.zeros(W * H, np.float32) if variance else None
        tail = (out.ctypes.data_as(C.POINTER(capi.rt_pixel)),
                None if var is None else var.ctypes.data_as(C.POINTER(C.c_float)))
        head = (film.ctypes.data_as(C.POINTER(capi.rt_pixel)), mom.ctypes.data_as(C.POINTER(capi.rt_moment)),
                feat.ctypes.data_as(C.POINTER(capi.rt_feature)))
        if albedo is None:
            self._chk("rt_denoise", self.lib.rt_denoise(self.h, C.byref(d), W, H, *head, *tail))
        else:
            albedo = np.ascontiguousarray(albedo, np.float32)
            assert albedo.shape == (W * H, 4)
            self._chk("rt_denoise_albedo", self.lib.rt_denoise_albedo(
                self.h, C.byref(d), float(albedo_floor), W, H, *head, albedo.ctypes.data_as(C.POINTER(capi.rt_albedo)),
                *tail))
        return (out, var) if variance else out

    def adaptive_denoise(self, demodulate=False, albedo_floor=ALBEDO_FLOOR_DEFAULT, **desc):
        """rt_adaptive_denoise: the open session's film filtered on the device (features rendered once per session);
        the session is left as it was.  demodulate=True: rt_adaptive_denoise_albedo, with a session-owned albedo film
        rendered with the features."""
        d = self._denoise_desc(**desc)
        out = self.new_film()
        if demodulate:
            self._chk("rt_adaptive_denoise_albedo", self.lib.rt_adaptive_denoise_albedo(
                self.h, C.byref(d), float(albedo_floor), out.ctypes.data_as(C.POINTER(capi.rt_pixel))))
        else:
            self._chk("rt_adaptive_denoise", self.lib.rt_adaptive_denoise(self.h, C.byref(d),
                                                                          out.ctypes.data_as(C.POINTER(capi.rt_pixel))))
        return out

    def render_denoised(self, min_samples, step_samples, max_samples, rel_error, abs_floor=1e-3, demodulate=False,
                        albedo_floor=ALBEDO_FLOOR_DEFAULT, **desc):
        """Adaptive session -> denoise -> end: (filtered film, info dict of the session).  demodulate=True filters the
        film divided by its first-hit albedo, which keeps the detail of an albedo texture."""
        self.adaptive_begin(min_samples, step_samples, max_samples, rel_error, abs_floor)
        try:
            info = self.adaptive_step()
            while info["active_pixels"] > 0 and info["index_done"] < max_samples:
                info = self.adaptive_step()
            return self.adaptive_denoise(demodulate=demodulate, albedo_floor=albedo_floor, **desc), info
        finally:
            self.adaptive_end()

    # ---- temporal accumulation (rt_render_features_pos, rt_temporal_*) -------------------------
    @staticmethod
    def _temporal_desc(**kw):
        unknown = set(kw) - set(TEMPORAL_DEFAULTS) - set(CHAIN_DEFAULTS) - {"chain_curved"}
        if unknown:
            raise TypeError(f"unknown temporal parameters: {sorted(unknown)}")
        p = {**TEMPORAL_DEFAULTS, **CHAIN_DEFAULTS, **kw}
        d = capi.rt_temporal_desc()
        d.normal_min, d.plane_rel, d.max_history = float(p["normal_min"]), float(p["plane_rel"]), float(p["max_history"])
        d.feature_samples = int(p["feature_samples"])
        d.chain_depth = chain_arg(p["chain_depth"], p.get("chain_curved", CHAIN_CURVED_DEFAULT))
        return d

    @staticmethod
    def _matrix16(m):
        m = np.ascontiguousarray(m, np.float32).reshape(-1)
        assert m.shape == (16,), "a column-major 4x4 matrix (scene.world_to_film)"
        return m

    def render_features_pos(self, index_begin, index_end, feat=None, pos=None):
        """rt_render_features_pos: render_features that also accumulates the first-hit position film (hit point sums
        and hit count, float32 [W*H, 4]); returns (feat, pos)."""
        feat = self.new_film() if feat is None else feat
        pos = self.new_film() if pos is None else pos
        for a in (feat, pos):
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (self.res[0] * self.res[1], 4)
        self._chk("rt_render_features_pos", self.lib.rt_render_features_pos(
            self.h, index_begin, index_end, feat.ctypes.data_as(C.POINTER(capi.rt_feature)),
            pos.ctypes.data_as(C.POINTER(capi.rt_position))))
        return feat, pos

    def render_features_chain(self, index_begin, index_end, chain_depth, feat=None, pos=None, with_pos=True,
                              chain_curved=CHAIN_CURVED_DEFAULT):
        """rt_render_features_chain: render_features_pos whose samples follow mirrors and dielectrics for up to
        chain_depth continuation rays (0..capi.RT_CHAIN_MAX) and describe the end of that chain.
        Returns (feat, pos); with_pos=False: the feature film alone (pos_inout NULL), returns feat.
        chain_curved=True: the curvature-aware virtual distance (capi.RT_CHAIN_CURVED)."""
        feat = self.new_film() if feat is None else feat
        if with_pos:
            pos = self.new_film() if pos is None else pos
        for a in (feat, pos) if with_pos else (feat,):
            assert a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (self.res[0] * self.res[1], 4)
        self._chk("rt_render_features_chain", self.lib.rt_render_features_chain(
            self.h, index_begin, index_end, chain_arg(chain_depth, chain_curved), feat.ctypes.data_as(C.POINTER(capi.rt_feature)),
            pos.ctypes.data_as(C.POINTER(capi.rt_position)) if with_pos else None))
        return (feat, pos) if with_pos else feat

    def temporal_accumulate(self, film, mom, feat, pos, history=None, world_to_film_prev=None, res=None, **desc):
        """rt_temporal_accumulate on host arrays of `res` (default: the film's).  history: None, or the previous
        frame's (accumulated film, moments, features, positions), reprojected through world_to_film_prev.  Returns
        (out_film [N, 4], out_mom [N, 2], info dict).  Descriptor fields default to TEMPORAL_DEFAULTS."""
        W, H = res or self.res
        n = W * H
        cur = [np.ascontiguousarray(a, np.float32) for a in (film, mom, feat, pos)]
        assert [a.shape for a in cur] == [(n, 4), (n, 2), (n, 4), (n, 4)]
        types = [capi.rt_pixel, capi.rt_moment, capi.rt_feature, capi.rt_position]
        args = [a.ctypes.data_as(C.POINTER(t)) for a, t in zip(cur, types)]
        if history is None:
            hist, args, m = [], args + [None] * 4, None
        else:
            hist = [np.ascontiguousarray(a, np.float32) for a in history]
            assert [a.shape for a in hist] == [(n, 4), (n, 2), (n, 4), (n, 4)]
            args += [a.ctypes.data_as(C.POINTER(t)) for a, t in zip(hist, types)]
            m = self._matrix16(world_to_film_prev)
        d = self._temporal_desc(**desc)
        out, outm, info = np.zeros((n, 4), np.float32), np.zeros((n, 2), np.float32), capi.rt_temporal_info()
        self._chk("rt_temporal_accumulate", self.lib.rt_temporal_accumulate(
            self.h, C.byref(d), W, H, *args, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
            out.ctypes.data_as(C.POINTER(capi.rt_pixel)), outm.ctypes.data_as(C.POINTER(capi.rt_moment)),
            C.byref(info)))
        return out, outm, self._adaptive_info(info)

    def temporal_begin(self, **desc):
        """Open a temporal session: the history of the frames to come stays on the device."""
        self._chk("rt_temporal_begin", self.lib.rt_temporal_begin(self.h, C.byref(self._temporal_desc(**desc))))

    def temporal_frame(self, world_to_film, min_samples, step_samples=1, max_samples=None, rel_error=0.0,
                       abs_floor=1e-3, denoise=None, guided=False):
        """rt_temporal_frame of the current camera, whose matrix is world_to_film (scene.world_to_film): an adaptive
        frame (max_samples None: uniform, min_samples everywhere), accumulated against the session's history and,
        with denoise = a dict of rt_denoise_desc fields (may be empty: DENOISE_DEFAULTS), filtered.  Returns (film,
        info dict).  guided=True: rt_temporal_frame_guided, whose adaptive session estimates its block errors on the
        accumulated film; info["session"] is that session's rt_adaptive_info as a dict."""
        ad = self._adaptive_desc(min_samples, step_samples, min_samples if max_samples is None else max_samples,
                                 rel_error, abs_floor)
        dd = None if denoise is None else self._denoise_desc(**denoise)
        m = self._matrix16(world_to_film)
        out, info = self.new_film(), capi.rt_temporal_info()
        args = (self.h, C.byref(ad), None if dd is None else C.byref(dd), m.ctypes.data_as(C.POINTER(C.c_float)),
                out.ctypes.data_as(C.POINTER(capi.rt_pixel)), C.byref(info))
        if not guided:
            self._chk("rt_temporal_frame", self.lib.rt_temporal_frame(*args))
            return out, self._adaptive_info(info)
        session = capi.rt_adaptive_info()
        self._chk("rt_temporal_frame_guided", self.lib.rt_temporal_frame_guided(*args, C.byref(session)))
        return out, dict(self._adaptive_info(info), session=self._adaptive_info(session))

    def temporal_block_error(self, film, mom, feat, pos, history=None, world_to_film_prev=None, res=None,
                             rel_error=0.0, abs_floor=1e-3, **desc):
        """rt_temporal_block_error on host arrays of `res` (default: the film's): the block errors a guided frame's
        session estimates, k_adaptive_error of what temporal_accumulate gives for the same arguments.  Returns
        (block_error [rows, columns], converged [rows, columns] int32)."""
        W, H = res or self.res
        n = W * H
        cur = [np.ascontiguousarray(a, np.float32) for a in (film, mom, feat, pos)]
        assert [a.shape for a in cur] == [(n, 4), (n, 2), (n, 4), (n, 4)]
        types = [capi.rt_pixel, capi.rt_moment, capi.rt_feature, capi.rt_position]
        args = [a.ctypes.data_as(C.POINTER(t)) for a, t in zip(cur, types)]
        if history is None:
            hist, args, m = [], args + [None] * 4, None
        else:
            hist = [np.ascontiguousarray(a, np.float32) for a in history]
            assert [a.shape for a in hist] == [(n, 4), (n, 2), (n, 4), (n, 4)]
            args += [a.ctypes.data_as(C.POINTER(t)) for a, t in zip(hist, types)]
            m = self._matrix16(world_to_film_prev)
        d = self._temporal_desc(**desc)
        ad = self._adaptive_desc(rel_error=rel_error, abs_floor=abs_floor)
        bx, by = (W + 7) // 8, (H + 7) // 8
        err, conv = np.zeros((by, bx), np.float32), np.zeros((by, bx), np.int32)
        self._chk("rt_temporal_block_error", self.lib.rt_temporal_block_error(
            self.h, C.byref(d), C.byref(ad), W, H, *args, None if m is None else m.ctypes.data_as(C.POINTER(C.c_float)),
            err.ctypes.data_as(C.POINTER(C.c_float)), conv.ctypes.data_as(C.POINTER(C.c_int32))))
        return err, conv

    def temporal_reset(self):
        """Drop the session's history: the next frame is a first frame."""
        self._chk("rt_temporal_reset", self.lib.rt_temporal_reset(self.h))

    def temporal_end(self):
        self._chk("rt_temporal_end", self.lib.rt_temporal_end(self.h))

    def set_camera(self, camera):
        """rt_camera_set alone (allowed inside a temporal session)."""
        self._chk("rt_camera_set", self.lib.rt_camera_set(self.h, C.byref(camera.desc())))

    def resolve(self, film, srgb=False):
        """rt_film_resolve (the reference's linear 255·x) or rt_film_resolve_srgb (pbrt's sRGB encoding)."""
        out = np.zeros((self.res[0] * self.res[1], 3), np.uint8)
        name = "rt_film_resolve_srgb" if srgb else "rt_film_resolve"
        self._chk(name, getattr(self.lib, name)(self.h, np.ascontiguousarray(film, np.float32).ctypes.data_as(
            C.POINTER(capi.rt_pixel)), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def film_matrices(self):
        """(XYZFromSensorRGB, RGBFromXYZ) of the current film's sensor, column-major float32[9] each."""
        a, b = np.zeros(9, np.float32), np.zeros(9, np.float32)
        P = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        self._chk("rt_film_matrices", self.lib.rt_film_matrices(self.h, P(a), P(b)))
        return a, b

    def stats(self):
        s = capi.rt_stats()
        self._chk("rt_get_stats", self.lib.rt_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in s._fields_}

    def reset_stats(self):
        self._chk("rt_reset_stats", self.lib.rt_reset_stats(self.h))

    def octree(self):
        info = capi.rt_octree_info()
        self._chk("rt_octree_get_info", self.lib.rt_octree_get_info(self.h, C.byref(info)))
        n, r = info.n_nodes, info.n_leaf_refs
        b = np.zeros((n, 6), np.float32)
        ch, lf, lc = (np.zeros(n, np.int32) for _ in range(3))
        refs = np.zeros(max(r, 1), np.int32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk("rt_octree_export", self.lib.rt_octree_export(self.h, P(b, C.c_float), P(ch, C.c_int32), P(lf, C.c_int32),
                                                                P(lc, C.c_int32), P(refs, C.c_int32)))
        return dict(bounds=b, child=ch, leaf_first=lf, leaf_count=lc, refs=refs[:r], depth=info.depth,
                    max_queue_groups=info.max_queue_groups)

    def bvh(self, tile_set=0):
        """The fast traversal's BVH as uploaded (rt_bvh_export): nodes (n, 32) f32, tiles (m, 12) f32, consts."""
        return _bvh_arrays(lambda nn, nt, cs, nd, tl: self.lib.rt_bvh_export(self.h, tile_set, nn, nt, cs, nd, tl),
                           lambda rc: self._chk("rt_bvh_export", rc))

    def trace(self, ro, rd, use_cull=True):
        ro = np.ascontiguousarray(ro, np.float32)
        rd = np.ascontiguousarray(rd, np.float32)
        n = len(ro)
        prim = np.zeros(n, np.int32)
        bt = np.zeros((n, 4), np.float32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk("rt_debug_trace", self.lib.rt_debug_trace(self.h, n, P(ro, C.c_float), P(rd, C.c_float), int(use_cull),
                                                            P(prim, C.c_int32), P(bt, C.c_float)))
        return prim, bt

    def occluded(self, ro, rd, tmax):
        """Shadow query of the path kernels (any hit within tmax): int32 0/1 per ray."""
        ro = np.ascontiguousarray(ro, np.float32)
        rd = np.ascontiguousarray(rd, np.float32)
        tmax = np.ascontiguousarray(tmax, np.float32)
        occ = np.zeros(len(ro), np.int32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk("rt_debug_occluded", self.lib.rt_debug_occluded(self.h, len(ro), P(ro, C.c_float), P(rd, C.c_float),
                                                                  P(tmax, C.c_float), P(occ, C.c_int32)))
        return occ

    def debug_sort(self, which, S, shard_len, keys, slots=None, bits_a=3, bits_b=3):
        """rt_debug_sort: the ray (which 0) or NEE (which 1) coherence sort on a synthetic sharded queue; returns the
        output array (8 S int32: queue positions / slots at the sorted positions) and the rewritten shard lengths."""
        shard_len = np.ascontiguousarray(shard_len, np.int32)
        keys = np.ascontiguousarray(keys, np.uint32)
        assert len(shard_len) == capi.QUEUE_SHARDS and len(keys) == capi.QUEUE_SHARDS * S
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32)
        out = np.zeros(capi.QUEUE_SHARDS * S, np.int32)
        olen = np.zeros(capi.QUEUE_SHARDS, np.int32)
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))
        self._chk("rt_debug_sort", self.lib.rt_debug_sort(self.h, int(which), int(S), P(shard_len, C.c_int32),
                                                          P(keys, C.c_uint32), None if sl is None else P(sl, C.c_int32),
                                                          int(bits_a), int(bits_b), P(out, C.c_int32),
                                                          P(olen, C.c_int32)))
        return out, olen

    def samples(self, pixel_ids, indices):
        pixel_ids = np.ascontiguousarray(pixel_ids, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        out = (capi.rt_sample_record * len(pixel_ids))()
        P = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        self._chk("rt_debug_samples", self.lib.rt_debug_samples(self.h, len(pixel_ids), P(pixel_ids), P(indices), out))
        return out

    def close(self):
        if getattr(self, "h", None):
            self.lib.rt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def records_to_arrays(recs):
    """rt_sample_record array -> dict of numpy arrays (for bit-exact comparisons)."""
    raw = np.frombuffer(bytes(recs), dtype=np.float32).reshape(len(recs), 39)
    return dict(lam=raw[:, 0:8], pdf=raw[:, 8:16], ro=raw[:, 16:19], rd=raw[:, 19:22],
                prim=raw[:, 22].view(np.int32), b=raw[:, 23:26], t=raw[:, 26], L=raw[:, 27:35], rgb=raw[:, 35:38],
                weight=raw[:, 38])


def _bvh_arrays(call, check):
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    nn, nt = C.c_int(), C.c_int()
    cs = np.zeros(2, np.float32)
    check(call(C.byref(nn), C.byref(nt), P(cs), None, None))
    nodes = np.zeros((max(nn.value, 1), 32), np.float32)
    tiles = np.zeros((max(nt.value, 1), 12), np.float32)
    check(call(C.byref(nn), C.byref(nt), P(cs), P(nodes), P(tiles)))
    return dict(nodes=nodes[: nn.value], tiles=tiles[: nt.value], consts=cs)


def build_bvh_host(model, tile_set=0):
    """rt_debug_bvh_build: the upload's BVH built on the host from a scene.Model, without a device (CPU tests)."""
    lib = capi.load_library()
    sd = model.desc()

    def check(rc):
        if rc != capi.RT_OK:
            raise capi.RTError("rt_debug_bvh_build", rc, "bad scene")
    return _bvh_arrays(lambda nn, nt, cs, nd, tl: lib.rt_debug_bvh_build(C.byref(sd), tile_set, nn, nt, cs, nd, tl),
                       check)
