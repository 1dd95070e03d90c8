/* =====================================================================================================
 * rtmi355x.h — the drop-in C-ABI of the MI355X ray-tracing inner loop (librtmi355x.so).
 *
 * Replaces the in-process per-pass block of the reference application
 *     RayTracerTestApp::MainLoop  →  ThreadFunction / evaluate_pixel dispatch + wait
 *     (Applications/RayTracerTestApp.h:287-422)
 * which samples (sampler), generates camera rays (CameraBase::generateRay, Cameras.h:179/273-297),
 * traverses the triangle octree (Octtree_Model::Traverse, Octtree_Model.h:66-127), shades (Li lambda,
 * RayTracerTestApp.h:218-284) and accumulates sensor RGB into the Film (Film.h:11-20, :336-337).
 *
 * Plain C: pointers and sizes only.  All descriptors are deep-copied at upload; the caller owns every
 * buffer.  Every entry point returns 0 (RT_OK) or a negative rt_status and sets rt_last_error().
 * No C++ exception crosses this boundary.  One rt_ctx per host thread (calls on a context are
 * serialised by the caller).  The library needs an MI355X (gfx950): rt_create fails with
 * RT_E_NODEVICE when none is present — there is no CPU fallback.
 * ===================================================================================================*/
#ifndef RTMI355X_H
#define RTMI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 10

typedef enum {
    RT_OK = 0,
    RT_E_ARG = -1,      /* invalid argument / descriptor                                   */
    RT_E_HIP = -2,      /* HIP runtime error (message in rt_last_error)                    */
    RT_E_RCCL = -3,     /* reserved: collectives run in the caller (torch.distributed)     */
    RT_E_OOM = -4,      /* device or host allocation failed (std::bad_alloc is caught)     */
    RT_E_STATE = -5,    /* call order: scene/camera/sampler/film not set; internal error   */
    RT_E_NODEVICE = -6, /* no gfx950 device visible                                        */
    RT_E_LIMIT = -7     /* scene exceeds a compiled limit (e.g. BFS queue bound)           */
} rt_status;

typedef struct rt_ctx rt_ctx;

#define RT_MAX_DEVICES 16
#define RT_QUEUE_SHARDS 8   /* shards of the multi-level path queues (rt_debug_sort) */
/* rt_create ("device list"): n_devices <= 1 renders on `device`; n_devices > 1 renders every pass
 * on devices[0..n_devices) at once — pixel tiles interleaved over the devices (tile t -> device t mod n), the
 * caller's film on devices[0] (rt_render_pass_device) or on the host, owned pixels exchanged with peer copies
 * over xGMI.  The film is bit-identical to a one-device render.  A device may be listed more than once (tests). */
typedef struct {
    int device;        /* HIP device ordinal (n_devices <= 1)                             */
    int octree_build;  /* RT_OCTREE_BUILD_DEVICE (default) or RT_OCTREE_BUILD_HOST         */
    int n_devices;     /* 0 or 1: one device; 2..RT_MAX_DEVICES: devices[]                 */
    int devices[RT_MAX_DEVICES];
    int reserved[5];
} rt_options;
/* Where rt_scene_upload builds the octree (Octtree_Model.h:33-63): both give the reference's tree bit for bit. */
enum { RT_OCTREE_BUILD_DEVICE = 0, RT_OCTREE_BUILD_HOST = 1 };

/* Film pixel, layout-identical to `pixel {glm::vec3 rgbsum; float weightsum;}` (Film.h:6-9). */
typedef struct { float r, g, b, w; } rt_pixel;
/* Per-pixel moments of the adaptive film: with v = (r + g) + b of one sample's clamped sensor RGB,
 * sum = sum + v and sumsq = sumsq + v * v for every sample, in the film's index order (float32, nothing fused). */
typedef struct { float sum, sumsq; } rt_moment;

enum { RT_MAT_DIFFUSE = 0, RT_MAT_MIRROR = 1, RT_MAT_DIELECTRIC = 2, RT_MAT_ROUGH = 3, RT_MAT_CONDUCTOR = 4,
       RT_MAT_ROUGH_DIELECTRIC = 5 };
/* the metal of an RT_MAT_CONDUCTOR material, carried as a float in rt_material.sigmoid[0] */
enum { RT_METAL_AG = 0, RT_METAL_AL = 1, RT_METAL_AU = 2, RT_METAL_CU = 3 };
/* Build-defined material (the reference has none: Shading.h:1-21 is a comment stub).
 * DIFFUSE: Lambert R/π; MIRROR: perfect specular reflection scaled by R; R(λ) is an RGBSigmoidPolynomial
 *   (color.h:363-403): R(λ) = s(c0 λ² + c1 λ + c2).
 * DIELECTRIC: smooth Fresnel glass; eta > 0 is a constant IOR, eta == 0 selects the dispersive
 *   "glass-BK7" table (spectrum.cpp:2674-2691) with SampledWavelengths::TerminateSecondary (spectrum.h:302-310).
 * ROUGH (additive): an isotropic, reflection-only GGX (Trowbridge-Reitz) microfacet reflector, MIRROR
 *   spread into a lobe.  The roughness alpha travels in `eta` (rt_scene_upload: RT_E_ARG unless it is finite and in
 *   [0.01, 1]; below 0.01 the caller wants RT_MAT_MIRROR; an emissive material's eta is not read).  float32 in the order
 *   written, nothing fused; vectors local to the pbrt CoordinateSystem frame (ss, tt, n) of the shading-side normal n
 *   (v_local = (v.ss, v.tt, v.n), glm dots), wo = -ray direction, mu_o = wo.z; a = alpha, a2 = a a:
 *     D(h)      = 1 / ((pi a2) (t t)),  t = (h.x h.x + h.y h.y) / a2 + h.z h.z   (= a2 / (pi (h.z^2 (a2 - 1) + 1)^2) for a
 *                 unit h; the form that does not cancel at alpha = 0.01)
 *     Lambda(w) = (sqrtf(1 + (a2 (1 - w.z w.z)) / (w.z w.z)) - 1) / 2,  G1(w) = 1 / (1 + Lambda(w)),
 *     G2        = 1 / ((1 + Lambda(wo)) + Lambda(wi))   (height-correlated)
 *     f(wo, wi) = R(lambda) D(h) G2 / (4 mu_o mu_i), h = normalize(wo + wi), 0 when mu_i <= 0 or mu_o <= 0.  The "Fresnel"
 *                 term is the material's (or its texel's) sigmoid R(lambda) at every angle, as MIRROR is reflection
 *                 scaled by R: f is R(lambda) times one scalar fcos / mu_i, fcos = (D G2) / (4 mu_o).
 *     sampling: Heitz's visible normals as pbrt-v4 TrowbridgeReitzDistribution::Sample_wm on the disk point (dx, dy) =
 *       disk_concentric(u0, u1) of the vertex's bounce Get2D:
 *       wh = normalize(a wo.x, a wo.y, wo.z); T1 = wh.z < 0.99999f ? normalize(cross((0, 0, 1), wh)) : (1, 0, 0);
 *       T2 = cross(wh, T1); hh = sqrtf(1 - dx dx); s = (1 + wh.z) / 2; dy' = (1 - s) hh + s dy;
 *       pz = sqrtf(max(0, (1 - dx dx) - dy' dy')); nh = (T1 dx + T2 dy') + wh pz;
 *       h = normalize(a nh.x, a nh.y, max(1e-6f, nh.z)); wi = (2 (wo.h)) h - wo;
 *       pdf(wo, wi) = (G1(wo) D(h)) / (4 mu_o); the bounce weight f mu_i / pdf = R(lambda) wb, wb = G2 / G1(wo) in [0, 1];
 *       wi.z <= 0 or mu_o <= 0: no bounce, the path ends (single-scattering GGX loses that energy: 20 % of the samples
 *       at alpha 0.5 and normal incidence).
 *   In the path integrators a rough vertex draws what a Lambert vertex draws, in the same order (one Get2D per light,
 *   one for the bounce); its light terms hold f mu_i where Lambert's hold (R / pi) cos, for every kind of light, and its
 *   MIS weights pdf(wo, wi) where Lambert's hold cos / pi; the bounce multiplies beta by R(lambda) wb and hands
 *   pdf(wo, wi) to the next emitter hit or environment miss.  An albedo texture supplies R as for Lambert.
 *   RT_INTEGRATOR_REFERENCE never sees materials; the feature, position and chain passes end a chain on a rough surface,
 *   as on a Lambert one; rt_render_features_albedo demodulates it by A of its material or texel, as Lambert (exact: f
 *   is R(lambda) times a scalar).  Limits: no transmission, no anisotropy, no angle-dependent Fresnel on this material
 *   (RT_MAT_CONDUCTOR below has the conductor's; RT_MAT_ROUGH_DIELECTRIC the dielectric's, with transmission), no
 *   multiple-scattering compensation, no roughness textures.
 * CONDUCTOR (additive): a metal: ROUGH's GGX lobe with the exact unpolarised conductor Fresnel term of a
 *   measured complex index n + i k in place of R(lambda).  `eta` is the roughness alpha, with ROUGH's rule (RT_E_ARG
 *   unless finite and in [0.01, 1], "alpha" in rt_last_error); sigmoid[0] is the metal as a float (RT_METAL_AG = 0,
 *   RT_METAL_AL = 1, RT_METAL_AU = 2, RT_METAL_CU = 3); sigmoid[1] and sigmoid[2] must be 0; anything else is RT_E_ARG and
 *   the scene bound before stays.  An emissive material's type, eta and sigmoid are not validated or read.
 *   Optical constants: one dense table NK[4][471] of (n, k) pairs; entry j is the piecewise-linear value of the metal's
 *   two measured tables (56 (lambda, value) pairs each, 298.76-885.60 nm) at lambda = 360 + j, computed on the host in
 *   float32 with PiecewiseLinearSpectrum::Query's operations (the same interval search, t = (lambda - l[o]) /
 *   (l[o+1] - l[o]), (1 - t) v[o] + t v[o+1]) and uploaded once per context (15 KB).  Kernels read it at the dense
 *   spectra's index, (long)roundf(lambda) - 360, as D65 and the sensor bars are read.
 *   Fresnel: unpolarised, exact, real arithmetic; only + - * /, sqrtf and comparisons, float32 in the order written,
 *   nothing fused.  With c = fminf(fmaxf(wo.h, 0), 1), h = normalize(wo + wi):
 *     c2 = c c;  s2 = 1 - c2;  t0 = (n n - k k) - s2;  ab = sqrtf(t0 t0 + (4 (n n)) (k k));  t1 = ab + c2
 *     a  = sqrtf(fmaxf(0.5f (ab + t0), 0));  t2 = (2 a) c;  Rs = (t1 - t2) / (t1 + t2)
 *     t3 = c2 ab + s2 s2;  t4 = t2 s2;  Rp = (Rs (t3 - t4)) / (t3 + t4);  F = 0.5f (Rp + Rs)
 *   BSDF: f = F(lambda, wo.h) D(h) G2 / (4 mu_o mu_i); D, Lambda, G2, the frame, the visible-normal sampling, the pdf and
 *   wb = G2 / G1(wo) are ROUGH's; F replaces R(lambda) and is in no pdf and no MIS weight.  A conductor vertex is a rough
 *   vertex in its control flow (the same draws in the same order, the same acceptance tests, weights and prevPdf); light
 *   l adds ((beta F(lambda, ch_l)) Le) wgt, ch_l the clamped wo.h of the light's wi, and the bounce multiplies beta by
 *   F(lambda, ch_b) wb, ch_b that of the bounce's wi.  No texture binds to a conductor (rt_scene_set_textures: RT_E_ARG);
 *   its entry of the albedo table is (1, 1, 1), so rt_render_features_albedo leaves it un-demodulated (its colour
 *   depends on the angle); the feature, position and chain passes end a chain on it, as on ROUGH.  Limits: no smooth conductor
 *   (alpha < 0.01) in the specular bin, no tints or textures, no user-supplied n, k, no multiple-scattering compensation.
 * ROUGH_DIELECTRIC (additive): rough glass, the non-absorbing rough interface of Walter et al. 2007 with
 *   ROUGH's isotropic GGX.  `eta` is the index of the side the geometric normal points away from, as DIELECTRIC's, and
 *   must be finite and > 1; eta == 0 (dispersive BK7) is refused for this type.  sigmoid[0] is the roughness alpha with
 *   ROUGH's rule ([0.01, 1], "alpha" in rt_last_error); sigmoid[1] and sigmoid[2] must be 0; anything else is RT_E_ARG and
 *   the scene bound before stays.  An emissive material's fields are not validated or read.
 *   Vectors local to ROUGH's frame of the shading-side normal (wo.z > 0); er = front ? eta : 1 / eta.  Only + - * /, sqrtf
 *   and comparisons, float32 in the order written, nothing fused:
 *     F(c, er): c = fminf(fmaxf(c, 0), 1); s2t = (1 - c c) / (er er); 1 when s2t >= 1; ct = sqrtf(max(1 - s2t, 0));
 *               rp = (er c - ct) / (er c + ct); rs = (c - er ct) / (c + er ct); F = (rp rp + rs rs) / 2
 *     light (reflection side only; the cs > 0 test refuses a light below): with ROUGH's fcos, pdf and ch = the clamped
 *               wo.h of (wo, wi): fcosF = F(ch, er) fcos in the light weight, pdfF = F(ch, er) pdf in every power heuristic
 *     bounce:   one Get2D per light in list order, one Get2D for the disk point, then one Get1D u.  h = ROUGH's visible
 *               normal; c = wo.h; F = F(c, er).
 *               u < F: wi = (2 c) h - wo, none when wi.z <= 0; weight G2(wo, wi) / G1(wo); prevPdf = F (G1 D / (4 wo.z))
 *               else:  s2t = max(1 - c c, 0) / (er er); ct = sqrtf(max(1 - s2t, 0)); wt = -wo / er + (c / er - ct) h,
 *                      none unless wt.z < 0; weight (G2(wo, wt) / G1(wo)) / (er er), Lambda(wt) from wt.z^2;
 *                      prevPdf = 0 (the next emitter or environment hit counts in full); the next ray starts at p - nrm off
 *   Both weights are f |mu_i| / pdf of the whole BSDF (reflection F D G2 / (4 mu_o mu_i) plus Walter's transmission term)
 *   under "visible normal, then Fresnel choice"; the 1 / er^2 is DIELECTRIC's radiance scaling.  The reflection
 *   hemisphere is covered by NEE plus the sampled emitter or environment hit under the power heuristic with pdfF; the
 *   transmission hemisphere by the sampled direction alone.  No texture binds to it (RT_E_ARG); its albedo-table entry is
 *   (1, 1, 1); the feature, position and chain passes end a chain on it.  Limits: constant eta only, no absorption or
 *   tint of its own (a medium bound with rt_scene_set_media, DESIGN.md §3n, absorbs inside DIELECTRIC and
 *   ROUGH_DIELECTRIC solids), no NEE through the interface (delta lights reach the reflection lobe only, shadow rays stop at glass), single
 *   scattering, no roughness textures.
 * emission_scale > 0 makes the surface a pure one-sided emitter with Le = scale · stdillum-D65. */
typedef struct {
    int type;
    float sigmoid[3];
    float emission_scale;
    float eta;
} rt_material;

enum { RT_SHAPE_SPHERE = 0, RT_SHAPE_DISK = 1, RT_SHAPE_TRIANGLE = 2 };
/* Analytic shapes besides the triangle octree (Shapes.h:172-907), intersected in object space.
 * SPHERE: Sphere(r, zmin, zmax, phimax) (Shapes.h:209-432) — full spheres only (zmin <= -r, zmax >= r,
 *   phimax >= 360), so the atan2 φ clip can never fire;  DISK: Disk(height, inner, outer, phimax)
 *   (Shapes.h:622-758), phimax >= 360;  TRIANGLE: TriangleSimple(p1, p2, p3) (Shapes.h:760-907). */
typedef struct {
    int type;
    float object_to_render[16];      /* column-major rigidtransform * permutation_y_z (Shapes.h:175-181) */
    float render_to_object[16];      /* column-major glm::inverse(ObjectToRender)                        */
    float normal_to_render[9];       /* column-major mat3(transpose(inverse(ObjectToRender))) (:150)     */
    float radius, zmin, zmax, phimax;
    float height, inner_radius, outer_radius;
    float p[9];                      /* TriangleSimple p1, p2, p3 (object space) */
    int material;
} rt_shape;

enum { RT_LIGHT_QUAD = 0, RT_LIGHT_DISK = 1, RT_LIGHT_POINT = 2, RT_LIGHT_DISTANT = 3, RT_LIGHT_MESH = 4,
       RT_LIGHT_ENV = 5 };   /* ENV: the environment light's type on the device; bound with rt_scene_set_environment,
                                rejected (RT_E_ARG) in a light list */
/* Build-defined lights (Lights.h:1-10 is a comment stub naming area, point and sun lights).
 * QUAD: x = p + u·e1 + v·e2, emitting normal n, Le from `material` (the quad is also geometry: two
 *   emissive triangles of the mesh);  DISK: uniform area sampling of shapes[shape] (an emissive DISK
 *   shape with inner_radius 0), Le from its material;  POINT: at p, intensity scale · D65;
 *   DISTANT: unit direction `dir` towards the light, irradiance scale · D65.
 * MESH (reads `material` only): the light is every non-degenerate mesh triangle whose tri_material is
 *   `material`, in ascending triangle id, sampled uniformly by area (one sample and one shadow ray per
 *   path vertex whatever the triangle count).  Each triangle emits from the side of its geometric normal
 *   normalize(cross(p0 - p2, p1 - p2)) of its world vertices; Le from the material.  rt_scene_upload
 *   returns RT_E_ARG when the material is out of range or not emissive, when no non-degenerate triangle
 *   uses it, when an analytic shape uses it, or when another light names the same material.
 *   RT_INTEGRATOR_REFERENCE ignores it, like every light. */
typedef struct {
    int type;
    float p[3], e1[3], e2[3], n[3];
    float dir[3];
    float scale;
    int shape;
    int material;
} rt_light;

/* TriModel + Octtree_Model inputs (Shapes.h:1272-1491, Octtree_Model.h:33-63). */
typedef struct {
    int n_vertices;
    const float* positions;          /* object space, 3 floats per vertex (MeshCache::Mesh::positions) */
    const float* normals;            /* object space vertex normals (MeshCache::Mesh::normals)        */
    int n_triangles;
    const uint32_t* indices;         /* 3 per triangle                                                 */
    float object_to_render[16];      /* column-major; = rigidtransform * permutation_y_z (Shapes.h:180) */
    float normal_to_render[9];       /* column-major mat3(transpose(inverse(ObjectToRender))) (:1364)   */
    int cull_backfaces;              /* TriModel::ComputeBackFace(look, enable) (Shapes.h:1339-1380)    */
    float cull_look[3];
    int octree_capacity;             /* TRIANGLE_CAPACITY (Octtree_Model.h:388); 0 -> 40                */
    const int32_t* tri_material;     /* per triangle material id, NULL -> 0 (path integrator only)     */
    int n_materials;
    const rt_material* materials;
    int n_lights;
    const rt_light* lights;
    int n_shapes;                    /* analytic shapes, intersected after the octree in list order     */
    const rt_shape* shapes;
} rt_scene_desc;

enum { RT_CAMERA_PERSPECTIVE = 0, RT_CAMERA_ORTHOGRAPHIC = 1, RT_CAMERA_PINHOLE = 2, RT_CAMERA_THINLENS = 3 };
/* The values CameraBase and its subclasses already hold (Cameras.h:190-210 and the members below).
 * PERSPECTIVE: generateRay Cameras.h:273-297 (raster_to_camera, lens_radius, focal_distance);
 * ORTHOGRAPHIC: Cameras.h:230-243 (raster_to_camera);
 * PINHOLE: Cameras.h:328-339, the sampler overload (raster_to_screen, pinhole_depth = box_dimensions.z);
 * THINLENS: Cameras.h:378-400 (raster_to_screen, thin_focal = R/2, thin_aperture_diameter = lens_d - apeture,
 *   sensor_depth); the reference only offers a (lens_angle, len_percent_r) overload, so the build draws one
 *   Get2D per sample: lens_angle = 360° · u0, len_percent_r = u1. */
typedef struct {
    int type;
    float raster_to_camera[16];      /* column-major M_RastertoCamera */
    float camera_to_world[16];       /* column-major M_CameratoWorld  */
    float lens_radius;
    float focal_distance;
    float raster_to_screen[16];      /* column-major M_RastertoScreen (Cameras.h:93-94) */
    float pinhole_depth;
    float thin_focal;
    float thin_aperture_diameter;
    float sensor_depth;
} rt_camera_desc;

enum { RT_SAMPLER_INDEPENDENT = 0, RT_SAMPLER_STRATIFIED = 1, RT_SAMPLER_SOBOL = 2 };
enum { RT_SOBOL_NONE = 0, RT_SOBOL_PERMUTE_DIGITS = 1, RT_SOBOL_FAST_OWEN = 2, RT_SOBOL_OWEN = 3 };
/* pbrt::IndependentSampler(spp, seed) (samplers.h:38-62): x_samples = spp, y_samples ignored.
 * pbrt::StratifiedSampler(x, y, jitter, seed) (samplers.h:66-136).
 * pbrt::SobolSampler(spp, film resolution, randomize, seed) (samplers.h:227-327): x_samples = spp.  The
 * reference declares SobolMatrices32 without defining it (HelperFunctions.h:208-210); the build generates the
 * generator matrices for 32 dimensions from the Joe-Kuo direction numbers (dimensions >= 32 wrap to 2 as in
 * samplers.h:270-283) and derives SobolIntervalToIndex's VdC tables itself (equal to HelperFunctions.h:212-470). */
typedef struct {
    int kind;
    int x_samples, y_samples;
    int jitter;
    int seed;
    int randomize;                   /* Sobol: RT_SOBOL_* */
} rt_sampler_desc;

enum { RT_FILTER_BOX = 0, RT_FILTER_TRIANGLE = 1, RT_FILTER_GAUSSIAN = 2, RT_FILTER_LANCZOS = 3 };
/* PixelSensor (pixelsensor.h:37-79).  RT_SENSOR_XYZ: r/g/b = CIE X/Y/Z, XYZFromSensorRGB = WhiteBalance(sensor
 * illuminant white -> sRGB white).  1..17: the camera response curves the reference names in spectrum.cpp
 * (rt_sensor_name), XYZFromSensorRGB fitted over the 24 Macbeth swatches under the sensor illuminant exactly as
 * pixelsensor.h:37-68 does it (glm column-major LinearLeastSquares, helpers.h:258-272). */
enum { RT_SENSOR_XYZ = 0, RT_SENSOR_CANON_EOS_100D = 1, RT_SENSOR_COUNT = 18 };
/* Named illuminants of Spectra::Init (spectrum.cpp:2620-2637, all Y-normalised): the sensor illuminant. */
enum {
    RT_ILLUM_D65 = 0, RT_ILLUM_A = 1, RT_ILLUM_D50 = 2, RT_ILLUM_F1 = 3, /* F1..F12 = 3..14 */
    RT_ILLUM_ACES_D60 = 15, RT_ILLUM_COUNT = 16
};
/* Film (Film.h:11-20) + its filter + XYZ PixelSensor (pixelsensor.h:70-87).  Filters: Box (filters.h:66-93),
 * Triangle (267-296, deterministic coin), Gaussian (96-154, sigma = filter_param) and LanczosSinc (223-264,
 * tau = filter_param), the last two sampled through the reference's tabulated Continuous_Inversion_Sampler
 * (Sampling.h:781-877; 10000 / 2000 bins) driven by the sampler's GetPixel2D. */
typedef struct {
    int res_x, res_y;
    int filter;
    float filter_radius[2];
    float imaging_ratio;             /* 1/CIE_Y_integral in the reference app (RayTracerTestApp.h:149) */
    float filter_param;              /* Gaussian sigma (0 -> 0.5) / Lanczos tau (0 -> 3)               */
    int sensor;                      /* RT_SENSOR_XYZ or a camera (1..RT_SENSOR_COUNT-1)               */
    int sensor_illum;                /* RT_ILLUM_*: sensorIllum of the PixelSensor constructors        */
} rt_film_desc;

enum { RT_INTEGRATOR_REFERENCE = 0, RT_INTEGRATOR_PATH = 1, RT_INTEGRATOR_PATH_MIS = 2 };
/* RT_INTEGRATOR_REFERENCE: the Li lambda of RayTracerTestApp.h:218-284 (ambient 0.3·F1 +
 *   clamp(n·(0,0,-1))·D65·albedo), octree back-face culling honoured.
 * RT_INTEGRATOR_PATH: build-defined path tracer (Integrator.h:1-14 is a stub): one light
 *   sample per light at every diffuse vertex (NEE), emitters seen by camera rays or specular bounces.
 * RT_INTEGRATOR_PATH_MIS: the same plus BSDF-sampled emitter hits, both weighted by the power heuristic. */
typedef struct {
    int kind;
    int max_depth;
    float albedo_rgb[3];             /* reference Li material colour (grey: color.cpp:35-37 branch) */
} rt_integrator_desc;

typedef struct {
    int64_t samples;                 /* camera samples evaluated                         */
    int64_t rays;                    /* closest-hit rays traced                          */
    int64_t shadow_rays;             /* any-hit rays traced                              */
    int64_t nodes_tested;            /* box tests executed by closest-hit rays (BVH child boxes, plus octree
                                        nodes of BFS-traced rays)                        */
    int64_t tris_tested;             /* triangle tests executed by closest-hit rays      */
    int64_t shadow_nodes_tested;     /* node box tests by any-hit (shadow) rays          */
    int64_t shadow_tris_tested;      /* triangle tests by any-hit (shadow) rays          */
    int64_t hits;                    /* closest-hit rays that hit                        */
    double ms_generate, ms_trace, ms_shade, ms_shadow, ms_film;  /* HIP-event kernel time (0 with
                                        RTMI_NO_STAGE_EVENTS); ms_shadow is the deferred NEE kernel of mixed
                                        scenes or the shadow-queue kernel (RTMI_SHADOW_QUEUE=1), else 0: the
                                        simple path traces its shadow rays inside the shade kernel */
    int64_t launches_trace;          /* closest-hit trace launches (per-launch averages) */
    int64_t launches_shade;          /* shade launches (path mode: includes the inline shadow rays) */
    int64_t fallback_rays;           /* multi-level octrees: closest-hit rays the fast BVH traversal found
                                        ambiguous (canonical rule), traced by the reference BFS */
    int64_t shadow_fallback_rays;    /* the same for any-hit (shadow) rays                */
    double ms_sort;                  /* multi-level octrees: coherence sort of bounce rays (HIP events)  */
    int64_t nee_vertices;            /* mixed scenes: path vertices whose light samples k_path_nee traced */
    int64_t coop_overflows;          /* multi-level octrees: rays whose wave-cooperative BFS ran out of FIFO while the
                                        octree's exact queue bound promised it could not (DevScene coop_ok); always 0
                                        unless that bound is wrong — the tests require 0 */
} rt_stats;   /* multi-device contexts: every field summed over the devices */

/* Per-sample record for parity (stage outputs of one (pixel, index) camera sample). */
typedef struct {
    float lambda[8], pdf[8];
    float ro[3], rd[3];
    int32_t prim;
    float b[3], t;
    float L[8];
    float rgb[3];
    float weight;
} rt_sample_record;

/* Flattened octree as uploaded (node order = reference creation order, Octtree_Model.h:351). */
typedef struct {
    int n_nodes;
    int n_leaf_refs;
    int max_queue_groups;            /* host-computed bound of the BFS group queue       */
    int depth;
    int bvh_nodes;                   /* multi-level octrees: 4-wide nodes of the fast traversal's BVH (0: none) */
    int bvh_depth;
} rt_octree_info;

/* ---- lifecycle ---------------------------------------------------------------------------------- */
int rt_create(const rt_options* opt, rt_ctx** out);
void rt_destroy(rt_ctx* ctx);
const char* rt_last_error(const rt_ctx* ctx);
int rt_abi_version(void);

/* ---- configuration (each deep-copies its descriptor) -------------------------------------------- */
int rt_scene_upload(rt_ctx* ctx, const rt_scene_desc* scene);
int rt_camera_set(rt_ctx* ctx, const rt_camera_desc* cam);
int rt_sampler_set(rt_ctx* ctx, const rt_sampler_desc* smp);
int rt_film_set(rt_ctx* ctx, const rt_film_desc* film);
int rt_integrator_set(rt_ctx* ctx, const rt_integrator_desc* integ);
/* Pixel-tile sharding for multi-GPU: this context renders tiles t with t % n_shards == shard_id
 * (tile_size x tile_size pixel tiles in row-major tile order).  Default: one shard. */
int rt_set_shard(rt_ctx* ctx, int tile_size, int n_shards, int shard_id);

/* ---- the hot path ----------------------------------------------------------------------------- */
/* Accumulate (+=) sample indices [index_begin, index_end) of every owned pixel into film_inout
 * (res_x*res_y rt_pixel, host memory), index-ordered per pixel exactly as the reference's passes
 * (RayTracerTestApp.h:336-337, 420-422).  Blocks until done. */
int rt_render_pass(rt_ctx* ctx, int index_begin, int index_end, rt_pixel* film_inout);
/* Same, into a device-resident film (res_x*res_y rt_pixel in HBM) on the given hipStream_t
 * (NULL = the context's stream).  Returns after enqueueing; the caller synchronises. */
int rt_render_pass_device(rt_ctx* ctx, int index_begin, int index_end, void* d_film, void* hip_stream);

/* ---- adaptive sampling ---------------------------------------------------------- */
/* A session renders sample indices only where an error estimate is still high.  The unit is the image-aligned 8x8
 * pixel block: block error E = (sum of the pixels' standard errors of the mean) / (sum of their means + abs_floor),
 * converged when E <= rel_error; a converged block's pixels leave the active list for good.  Every active pixel
 * holds exactly the indices [0, film.w).  One-device contexts only. */
typedef struct {
    int min_samples;                 /* indices of the first step (>= 2)                                  */
    int step_samples;                /* indices of every later step (>= 1)                                */
    int max_samples;                 /* no pixel takes more (>= min_samples, <= the sampler's spp)        */
    float rel_error;                 /* threshold on E (>= 0, finite)                                     */
    float abs_floor;                 /* added to the block's mean sum (>= 0, finite)                      */
    int reserved[3];
} rt_adaptive_desc;
typedef struct {
    int iterations;                  /* steps that rendered                                               */
    int index_done;                  /* every active pixel holds indices [0, index_done)                  */
    int active_pixels;               /* pixels still in the active list                                   */
    int active_blocks;               /* 8x8 blocks not converged at the last estimate                     */
    int64_t samples;                 /* camera samples rendered by the session                            */
} rt_adaptive_info;
/* Zeroed device film and moments, every owned pixel active.  RT_E_STATE: a session is already open, or the
 * context has more than one device.  rt_film_set and rt_set_shard return RT_E_STATE while a session is open. */
int rt_adaptive_begin(rt_ctx* ctx, const rt_adaptive_desc* desc);
/* The next min_samples (first step) or step_samples indices, clipped to max_samples, on the active pixels; then the
 * block errors and the compaction of the active list.  Nothing active or index_done == max_samples: renders
 * nothing.  info may be NULL.  Blocks until done. */
int rt_adaptive_step(rt_ctx* ctx, rt_adaptive_info* info);
/* Copy out the session's state: film and mom (res_x*res_y each), block_error (ceil(res_x/8)*ceil(res_y/8), row-major
 * blocks; all 0 before the first step), the active pixel ids (up to the owned pixel count) and their number.  Any
 * pointer may be NULL. */
int rt_adaptive_read(rt_ctx* ctx, rt_pixel* film, rt_moment* mom, float* block_error, int32_t* active, int* n_active);
int rt_adaptive_end(rt_ctx* ctx);
/* begin; step until nothing is active or index_done == max_samples; read; end.  Outputs may be NULL. */
int rt_render_adaptive(rt_ctx* ctx, const rt_adaptive_desc* desc, rt_pixel* film_out, rt_moment* mom_out,
                       rt_adaptive_info* info);
/* The error estimate and the compaction alone, once, on caller-supplied host film and moments (res_x*res_y each) for
 * the current film and shard, starting from the full list of owned pixels (only rel_error and abs_floor of desc are
 * read).  Outputs as in rt_adaptive_read; any may be NULL. */
int rt_debug_adaptive_select(rt_ctx* ctx, const rt_adaptive_desc* desc, const rt_pixel* film, const rt_moment* mom,
                             float* block_error, int32_t* active, int* n_active);

/* ---- denoiser ------------------------------------------------------------------- */
/* First-hit guide image: per pixel the sums, over the samples of a feature pass, of the shading-side geometric
 * normal and the hit distance t of the camera rays that hit (misses add nothing, so |n| / samples is coverage). */
typedef struct { float nx, ny, nz, depth; } rt_feature;   /* 16 B, sums over the pass's samples */
/* Accumulate (+=) the features of sample indices [index_begin, index_end) of every owned pixel into feat_inout
 * (res_x*res_y, host memory): the camera rays of rt_render_pass traced as the current integrator's first trace
 * (same tile set, same analytic shapes), index-ordered per pixel.  Allowed while an adaptive session is open (always
 * the full work list).  Counts rays in rt_stats, not samples.  RT_E_STATE on multi-device contexts.  Blocks. */
int rt_render_features(rt_ctx* ctx, int index_begin, int index_end, rt_feature* feat_inout);
/* Variance-guided edge-avoiding a-trous filter (spatial SVGF): float32 in a fixed operation order, exp(-x) replaced
 * by max(1 - x/8, 0)^8 (three squarings).  Pixels need film.w >= 2 to carry a variance. */
typedef struct {
    int iterations;         /* 1..6; step of iteration i is 2^i                      */
    int feature_samples;    /* k >= 1: indices accumulated in feat                    */
    int normal_power_log2;  /* 0..8: w_n = max(0, n_p.n_q)^(2^j), by j squarings      */
    float sigma_l, sigma_z; /* > 0, finite                                            */
    float lum_floor;        /* >= 0, finite; added to sigma_l*sqrt(var)               */
    float depth_floor;      /* >= 0, finite; times z_p, added to the depth denominator */
    int chain_depth;        /* 0..RT_CHAIN_MAX [| RT_CHAIN_CURVED]: the sessions' guides, rt_render_features_chain */
} rt_denoise_desc;          /* 32 B */
/* Filter host arrays of any res_x x res_y (film, mom, feat, out: res_x*res_y each; variance_out: res_x*res_y floats
 * or NULL): out = (filtered mean * film.w, film.w), so both resolves apply.  The context supplies the device, the
 * stream and a workspace.  RT_E_ARG: bad descriptor, NULL array, or out overlapping an input.  Blocks. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_desc* desc, int res_x, int res_y, const rt_pixel* film, const rt_moment* mom,
               const rt_feature* feat, rt_pixel* out, float* variance_out);
/* Inside an adaptive session: the features of indices [0, feature_samples) at chain_depth (rendered once per session
 * into a device buffer, again when either changes), then the filter over the session's device film and moments into
 * film_out (res_x*res_y, host).  The session's film and moments are not modified. */
int rt_adaptive_denoise(rt_ctx* ctx, const rt_denoise_desc* desc, rt_pixel* film_out);

/* ---- temporal accumulation ------------------------------------------------------- */
/* First-hit position film: per pixel the sums, over the hits of a feature pass, of the render-space hit point
 * o + t d (per component, nothing fused) and the number of hits (a miss adds nothing). */
typedef struct { float x, y, z, hits; } rt_position;      /* 16 B, sums over the pass's hits */
/* rt_render_features that also accumulates (+=) the position film pos_inout (res_x*res_y, host memory) of the same
 * first hits; feat_inout comes out exactly as rt_render_features leaves it. */
int rt_render_features_pos(rt_ctx* ctx, int index_begin, int index_end, rt_feature* feat_inout, rt_position* pos_inout);
/* Specular-chain guides: rt_render_features_pos (pos_inout may be NULL: the feature film alone) whose
 * samples follow perfect mirrors and smooth dielectrics for up to chain_depth continuation rays (0..RT_CHAIN_MAX, else
 * RT_E_ARG) and describe the end of that chain.  Per sample, float32, nothing fused:
 *   the camera ray (o0, d0) is traced as in rt_render_features (a miss adds nothing); D = t0;
 *   at each hit the path integrator's surface: stop on an emitter (checked first), on a diffuse material, or after
 *   chain_depth continuations; otherwise the ray the integrator would spawn, offset 1e-4 (1 + max |p|) along the
 *   shading-side normal n: the reflection off a mirror (n is appended to a list N), through a dielectric the
 *   refraction whenever it exists (eta, or glass-BK7 at 550 nm when eta is 0; no sampler draw; nothing appended) and
 *   the reflection on total internal reflection; it is traced as a path bounce (every triangle, every analytic
 *   shape; a miss: the sample adds nothing) and D += t;
 *   feat += (v, D), v the last hit's normal reflected about the entries of N from last to first, and
 *   pos += (o0 + D d0, 1): the virtual point on the camera ray, exact for planar mirrors.
 * chain_depth 0, or the reference integrator (no materials: every chain has length 0), gives rt_render_features_pos'
 * films bit for bit.  Batches, shards, sessions, rt_stats (continuation rays count as rays) and RT_E_STATE on
 * multi-device contexts as rt_render_features.
 *
 * chain_depth | RT_CHAIN_CURVED (here and in rt_denoise_desc.chain_depth and rt_temporal_desc.chain_depth; any other
 * value outside 0..RT_CHAIN_MAX is RT_E_ARG; 0 | RT_CHAIN_CURVED behaves as 0): the curvature-aware virtual distance.
 * Everything above is unchanged except the D of feat and pos.  Each continuation surface k = 0..K-1 records
 * c_c = -(d.n), for a refraction c_f = -(wt.n) and mu = the far side's index over the camera side's (mu = 0 marks a
 * reflection), and the signed curvature kappa: +-1 / (radius sigma) for a sphere whose object_to_render linear part
 * is a rotation times a uniform scale sigma (decided in float64 at upload: G = L^T L, sigma^2 = tr G / 3,
 * max |G - sigma^2 I| <= 1e-5 sigma^2; rounded to float), + hit from outside, - from inside; 0 for every other
 * surface.  With t_k the length of the segment that reached surface k and t_K the last segment's, the chain's end
 * goes backwards from k = K-1 to 0 with s_T = s_S = 0, per plane u = t_(k+1) + s:
 *   reflection, kappa == 0:  s = u
 *   reflection:   a_T = 1 / u_T + (2 kappa) / c_c                              a_S = 1 / u_S + (2 kappa) c_c
 *   refraction:   a_T = (((mu c_f) c_f) / u_T + (c_c - mu c_f) kappa) / (c_c c_c)   a_S = mu / u_S + (c_c - mu c_f) kappa
 *   s = 1 / a
 * then D_T = t_0 + s_T, D_S = t_0 + s_S and D = ((2 D_T) D_S) / (D_T + D_S).  A sample keeps the plain sum D when
 * every record is a reflection with kappa == 0 (bit for bit the films without the flag) or when some a is not > 0 (the
 * image is real, at infinity, or NaN: inside a concave mirror).  The tangential and the sagittal plane are taken as
 * aligned along the chain: exact for one sphere, an approximation across several objects. */
#define RT_CHAIN_MAX 4
#define RT_CHAIN_CURVED 0x100
int rt_render_features_chain(rt_ctx* ctx, int index_begin, int index_end, int chain_depth, rt_feature* feat_inout,
                             rt_position* pos_inout);
/* Reprojection of the previous frame's accumulated film and moments through the previous camera, rejection of taps
 * whose geometry disagrees, and a sample-count-weighted running mean; float32 in a fixed operation order. */
typedef struct {
    float normal_min;       /* -1..1: a history tap needs n_p.n_q >= normal_min                              */
    float plane_rel;        /* >= 0, finite: and |n_p.(P_q - P)| <= plane_rel * depth                        */
    float max_history;      /* >= 1: cap of the accumulated sample count n'                                  */
    int feature_samples;    /* k >= 1: indices accumulated in the feature and position films                 */
    int chain_depth;        /* 0..RT_CHAIN_MAX [| RT_CHAIN_CURVED]: the frames' guides, rt_render_features_chain */
    int reserved[3];
} rt_temporal_desc;         /* 32 B */
typedef struct {
    int frames;             /* frames behind the history that was used (0: none, the outputs are the inputs)  */
    int reprojected;        /* pixels blended with their history                                              */
    int disoccluded;        /* pixels with a first hit and no usable history                                  */
    int background;         /* pixels whose feature pass hit nothing                                          */
} rt_temporal_info;         /* pixels with film.w == 0 are in no class */
/* The stage alone on host arrays of any res_x x res_y (res_x*res_y each): the current frame's film, moments, features
 * and positions, the previous frame's accumulated film and moments with its features and positions, and the previous
 * camera's world-to-film matrix (column-major; film space puts pixel (x, row) on [x, x+1) x [row, row+1)).  All four
 * hist_* NULL: no history (world_to_film_prev may be NULL too).  out = (mean * n', n') and (m1 * n', m2 * n'), an
 * ordinary film and moment film.  The context supplies the device, the stream and a workspace.  RT_E_ARG: bad
 * descriptor, NULL array, only some hist_* NULL, or an output overlapping an input.  info may be NULL.  Blocks. */
int rt_temporal_accumulate(rt_ctx* ctx, const rt_temporal_desc* desc, int res_x, int res_y, const rt_pixel* film,
                           const rt_moment* mom, const rt_feature* feat, const rt_position* pos,
                           const rt_pixel* hist_film, const rt_moment* hist_mom, const rt_feature* hist_feat,
                           const rt_position* hist_pos, const float* world_to_film_prev, rt_pixel* out_film,
                           rt_moment* out_mom, rt_temporal_info* info);
/* Frame session: the history (accumulated film and moments, features, positions: 56 B per pixel, ping-ponged) stays
 * on the device.  RT_E_STATE: a temporal or an adaptive session is already open, or the context has more than one
 * device.  While it is open rt_film_set, rt_set_shard, rt_adaptive_begin and rt_render_adaptive return RT_E_STATE;
 * rt_camera_set and the ordinary passes are allowed. */
int rt_temporal_begin(rt_ctx* ctx, const rt_temporal_desc* desc);
/* One frame of the current camera: an internal adaptive session by `adaptive` (uniform: min_samples == max_samples),
 * the features and positions of indices [0, feature_samples), the accumulation against the history, the a-trous filter
 * with the frame's features when `denoise` is not NULL (its feature_samples and chain_depth must equal the session's),
 * the result copied to film_out (res_x*res_y, host).  The unfiltered accumulation, the features, the positions and
 * world_to_film (this frame's camera) become the next frame's history.  info may be NULL.  Blocks. */
int rt_temporal_frame(rt_ctx* ctx, const rt_adaptive_desc* adaptive, const rt_denoise_desc* denoise,
                      const float* world_to_film, rt_pixel* film_out, rt_temporal_info* info);
/* rt_temporal_frame whose adaptive session estimates its block errors on the accumulated film.
 * session_info (may be NULL): the frame's internal adaptive session as rt_adaptive_step last reported it. */
int rt_temporal_frame_guided(rt_ctx* ctx, const rt_adaptive_desc* adaptive, const rt_denoise_desc* denoise,
                             const float* world_to_film, rt_pixel* film_out, rt_temporal_info* info,
                             rt_adaptive_info* session_info);
/* The guided estimate alone on host arrays of any res_x x res_y: k_temporal_reproject + k_temporal_error.  Inputs as
 * rt_temporal_accumulate (all four hist_* NULL: no history); only rel_error and abs_floor of `adaptive` are read.
 * block_error, converged: ceil(res_x/8)*ceil(res_y/8) each, row-major blocks; either may be NULL. */
int rt_temporal_block_error(rt_ctx* ctx, const rt_temporal_desc* desc, const rt_adaptive_desc* adaptive, int res_x,
                            int res_y, const rt_pixel* film, const rt_moment* mom, const rt_feature* feat,
                            const rt_position* pos, const rt_pixel* hist_film, const rt_moment* hist_mom,
                            const rt_feature* hist_feat, const rt_position* hist_pos, const float* world_to_film_prev,
                            float* block_error, int32_t* converged);
/* Drop the history (a cut, or a change of the scene): the next frame is a first frame. */
int rt_temporal_reset(rt_ctx* ctx);
int rt_temporal_end(rt_ctx* ctx);

/* a20 resolve (RayTracerTestApp.h:424-452): rgbsum/weightsum -> XYZFromSensorRGB -> sRGB -> clamp -> u8. */
int rt_film_resolve(rt_ctx* ctx, const rt_pixel* film, uint8_t* rgb_out);

/* a20 + pbrt ColorEncoding::sRGB (color.h:537-557, commented out in the reference): the same resolve, quantised with
 * LinearToSRGB8 (enoki minimax polynomial, round-to-nearest) instead of the reference's linear 255·x truncation. */
int rt_film_resolve_srgb(rt_ctx* ctx, const rt_pixel* film, uint8_t* rgb_out);

/* ---- scene ingest / image output / colour (host only: no device needed) ------------------------------- */
/* MeshCache::Mesh as the reference's assimp import leaves it (AssetManager.cpp:67-190): triangulated, one
 * vertex per face corner, file normals or flat face normals (aiProcess_GenNormals), texcoords or 0. */
typedef struct {
    int n_vertices;
    float* positions;                /* 3 per vertex */
    float* normals;                  /* 3 per vertex */
    float* texcoords;                /* 2 per vertex */
    int n_triangles;
    uint32_t* indices;               /* 3 per triangle */
} rt_mesh;
/* Wavefront OBJ (v / vt / vn / f, polygons fan-triangulated, negative indices) -> *out (free with rt_mesh_free). */
int rt_load_obj(const char* path, rt_mesh** out);
void rt_mesh_free(rt_mesh* mesh);
/* Write w x h 8-bit RGB to `path`: PNG when it ends in .png, binary PPM otherwise; flip_y writes rows bottom-up
 * (the film's row 0 is the image bottom: the reference uploads it as a GL texture, RayTracerTestApp.h:453-455). */
int rt_image_write(const char* path, int w, int h, const uint8_t* rgb, int flip_y);
/* RGBToSpectrumTable::operator() (color.cpp:26-72) for an sRGB reflectance in [0,1]^3: grey = the closed form of
 * color.cpp:35-37, otherwise the reference's trilinear lookup in the 3 x 64^3 coefficient table, which the build
 * regenerates (the reference's "../rgb2spec/sRGB64binary", color.cpp:114, is not in its repository; data/srgb64.rgbspec,
 * found next to the library or through RTMI_RGBSPEC_TABLE).  RT_E_STATE when the table is missing. */
int rt_rgb_to_sigmoid(const float* rgb, float* coeffs);
/* The table generator's per-entry solve for one colour: Gauss-Newton in CIELAB (rgb2spec_opt's method). */
int rt_rgb_fit_sigmoid(const float* rgb, float* coeffs);
/* Name of a PixelSensor (RT_SENSOR_XYZ -> "xyz", 1.. -> the reference's camera name), NULL when out of range. */
const char* rt_sensor_name(int sensor);
/* The film's resolve matrices (column-major, glm layout): XYZFromSensorRGB of the current sensor, sRGB RGBFromXYZ. */
int rt_film_matrices(rt_ctx* ctx, float* xyz_from_sensor9, float* rgb_from_xyz9);

/* ---- albedo textures ----------------------------------------------------------------- */
/* A diffuse or mirror material's reflectance R(lambda) read from an RGB8 image instead of the material's one sigmoid:
 * the reference's texture lookup (the `if (false)` branch of Li, RayTracerTestApp.h:229-242) on the uv of
 * Triangle::CalculateLocalSurface (Shapes.h:1036-1046).  float32, nothing fused:
 *   uv of a hit, per component: (tc1 b0 + tc2 b1) + tc3 b2, the hit's barycentrics over the corners' texcoords;
 *   texel: rt_texel_index (nearest; no filtering);
 *   albedo: rgb = byte / 255.f per channel, then rt_rgb_to_sigmoid; its (c0, c1, c2) replace the material's wherever
 *   the path integrators form R(lambda): the Lambert light terms, the Lambert bounce, the mirror scale.  Type, eta,
 *   emission and light binding stay the material's.
 * RT_INTEGRATOR_REFERENCE ignores textures (its Li has no materials); so do the feature, position and chain passes,
 * which read geometry only. */
enum { RT_TEX_CLAMP = 0, RT_TEX_REPEAT = 1 };
typedef struct {
    int width, height, wrap;         /* wrap: RT_TEX_CLAMP or RT_TEX_REPEAT                              */
    const uint8_t* rgb;              /* 3 bytes per texel, x fastest, row 0 is v = 0 (RayTracerTestApp.h:231) */
} rt_texture;
typedef struct {
    int n_textures;
    const rt_texture* textures;
    int n_materials;
    const int32_t* material_texture; /* per material of the uploaded scene (one entry for a scene uploaded without
                                        materials): texture id or -1                                        */
    int n_triangles;
    const float* tri_texcoords;      /* 6 per triangle: (u, v) of its three corners (the context keeps no index
                                        buffer: the caller gathers texcoords[indices])                      */
    int reserved[4];
} rt_texture_desc;
/* Bind textures to the uploaded scene (deep copy: the texels are baked to 16 B of coefficients each on the device, and
 * the 9.4 MB coefficient table is uploaded once per context).  NULL or n_textures == 0 clears them; rt_scene_upload
 * drops them.  A textured scene is shaded by the general path kernels (as a scene with MIS or several lights is).
 * RT_E_STATE: no scene, an adaptive or temporal session is open, a multi-device context, or the coefficient table is
 * missing.  RT_E_ARG: n_materials or n_triangles differ from the scene's, a texture id out of range, width or height
 * < 1, a NULL array, a bad wrap value, a texture bound to an emissive material or to a material an analytic shape uses
 * (shapes have no uv).  RT_E_LIMIT: n_materials plus the total texel count exceeds 2^31 - 1. */
int rt_scene_set_textures(rt_ctx* ctx, const rt_texture_desc* desc);
/* The texel a uv selects (host only, no context; RT_E_ARG for width or height < 1 or a bad wrap).  Per coordinate
 * CLAMP: u' = min(max(u, 0), 1) (Shapes.h:1045-1046); REPEAT: u' = u - floorf(u), and 0 when that is not < 1; a NaN
 * coordinate counts as 0 (build-defined).  x = (int)floorf(u' W) % W (u' = 1 wraps to column 0, as
 * RayTracerTestApp.h:234 does), y = min((int)floorf(v' H), H - 1) (the reference reads past the image at v = 1; the
 * clamp is build-defined); index = y W + x. */
int rt_texel_index(int width, int height, int wrap, float u, float v);
/* The bake kernel alone: n RGB8 texels (3n bytes) -> 3n floats (c0, c1, c2), bit for bit rt_rgb_to_sigmoid(byte / 255.f). */
int rt_debug_texture_bake(rt_ctx* ctx, int n, const uint8_t* rgb, float* coeffs);
/* The shade kernels' device function on n explicit (triangle id, b0 b1 b2): texel[i] = the texel index within its
 * texture, or -1 for an untextured triangle, and coeffs[3i..] = the (c0, c1, c2) the shade would use. */
int rt_debug_texture_eval(rt_ctx* ctx, int n, const int32_t* prim, const float* b, int32_t* texel, float* coeffs);

/* ---- mesh area lights (additive): RT_LIGHT_MESH above -------------------------------
 * The device table of mesh light `light` of the uploaded scene, built in float32 with nothing fused: with
 * cr = cross(p0 - p2, p1 - p2) (each component a*b - c*d as written there, the dot (x x + y y) + z z),
 * area_i = 0.5f sqrtf(dot(cr, cr)); S = the inclusive prefix sums of the areas taken 64 entries at a time (inside a
 * chunk v += shift_up(v, o) for o = 1, 2, 4, 8, 16, 32, entries below o keep theirs; S_i = carry + v, carry = the S of
 * the previous chunk's last entry, 0 for the first chunk); cdf_i = S_i / S_{n-1}.
 * *n = the triangle count and *area = S_{n-1} are always written; tri (n triangle ids), cdf (n) when non-NULL.
 * RT_E_ARG if `light` is not a mesh light of the scene. */
int rt_debug_meshlight_table(rt_ctx* ctx, int light, int* n, int32_t* tri, float* cdf, float* area);
/* The path kernels' own light-sampling device function for light `light` on n explicit shading points po (3n) and
 * sample points u (2n): wi (3n) the unit direction of the shadow ray, tmax, dist2 (n), nl (3n) the light's normal at
 * the sample and tri (n) the sampled triangle id (-1 and the light's n for the other light types).
 * A mesh light, float32 in the order written: i = the smallest index with u0 < cdf_i; lo = i > 0 ? cdf_{i-1} : 0;
 * u' = fminf((u0 - lo) / (cdf_i - lo), 0x1.fffffep-1f); if u' < u1: b0 = u' / 2, b1 = u1 - b0, else b1 = u1 / 2,
 * b0 = u' - b1; b2 = (1 - b0) - b1; pl = (p0 b0 + p1 b1) + p2 b2; nl = normalize(cross(p0 - p2, p1 - p2));
 * wv = pl - po, dist2 = dot(wv, wv), wi = wv (1 / sqrtf(dist2)), tmax = sqrtf(dist2) 0.999f. */
int rt_debug_light_sample(rt_ctx* ctx, int light, int n, const float* po, const float* u, float* wi, float* tmax,
                          float* dist2, float* nl, int32_t* tri);

/* ---- image environment light (additive) -------------------------------------------
 * One HDR map lights the scene from infinity: W x H texels of linear-sRGB float32 RGB (finite, >= 0), texel (x, y) at
 * index y W + x, laid over the unit square (s, t) by the plain octahedral mapping, with a rotation world_to_env (3x3,
 * column-major, glm operation order) and a scalar scale.  Build-defined; float32 in the order written, nothing fused.
 *   direction -> texel: e = M d; a = (|e.x| + |e.y|) + |e.z|; px = e.x / a, py = e.y / a; if e.z < 0:
 *     (px, py) = ((1 - |py|) copysignf(1, px), (1 - |px|) copysignf(1, py)) (the old values on the right);
 *     s = px 0.5f + 0.5f, t = py 0.5f + 0.5f; x = min((int)(s W), W - 1), y = min((int)(t H), H - 1); a NaN
 *     coordinate counts as 0 (as rt_texel_index).
 *   (s, t) -> direction: px = 2 s - 1, py = 2 t - 1, z = (1 - |px|) - |py|; if z < 0 the same fold; p = (px, py, z);
 *     d = M^T normalize(p).
 *   solid angle: d omega = 4 ds dt / |p|^3, so pdf_omega = (pdf_st (l2 sqrtf(l2))) / 4 with l2 = dot(p, p).
 *   emission (pbrt-v4 RGBIlluminantSpectrum, D65): per texel m = 2 max(r, g, b), (c0, c1, c2) = rt_rgb_to_sigmoid(rgb / m)
 *     (a black texel: m = 0); Le(lambda) = ((scale m) s(c0 lambda^2 + c1 lambda + c2)) D65(lambda).
 *   distribution: piecewise constant over texels, weight max(r, g, b) / (l2c sqrtf(l2c)) with l2c = dot(p, p) at the
 *     texel centre; per row the inclusive prefix sums in rt_debug_meshlight_table's scan order divided by the row total
 *     (a zero row: all 0), the row totals scanned and divided the same way into the marginal.
 *   sampling: one Get2D (u0, u1) per path vertex, the light being the last of the list: y = the smallest row with
 *     u1 < marg_y, x = the smallest column with u0 < cond_x of that row, both remapped as rt_debug_light_sample's u';
 *     s = (x + u0') / W, t = (y + u1') / H; pdf_st = ((cond_x - cond_{x-1}) (marg_y - marg_{y-1})) (float)(W H);
 *     tmax = FLT_MAX; the sample counts when cos > 0 and pdf_omega > 0, weight cos / pdf_omega, under PATH_MIS times
 *     the power heuristic of (pdf_omega, cos / pi).
 *   misses: a ray of the path integrators that leaves the scene adds beta Le(d) when it is a camera ray or follows a
 *     mirror or glass bounce, under PATH_MIS times the power heuristic of (the bounce's pdf, pdf_omega(d)) after a
 *     diffuse bounce, and nothing after a diffuse bounce without MIS.  Camera rays see the map as background.
 * RT_INTEGRATOR_REFERENCE and the feature, position and chain passes ignore the map: a miss there stays a miss.
 * Limits: nearest texel, one map, W H <= 2^24, one sample per path vertex like every light. */
typedef struct {
    int width, height;
    const float* rgb;                /* width * height * 3 floats                                          */
    float scale;
    float world_to_env[9];
    int reserved[4];
} rt_environment_desc;
/* Binds the map to the uploaded scene as one more light at the end of its list (deep copy; baked and tabulated on
 * every device of the context); NULL or width == 0 clears it; rt_scene_upload drops it.  RT_E_STATE: no scene, an open
 * adaptive or temporal session, or the coefficient table is missing.  RT_E_ARG: a size < 1, NULL rgb, a negative or
 * non-finite texel or scale, a map whose weights sum to 0 or to no finite float, or a full light list.  RT_E_LIMIT:
 * width * height > 2^24.  A rejected call leaves the scene and a map bound before as they were. */
int rt_scene_set_environment(rt_ctx* ctx, const rt_environment_desc* desc);
/* The texel a direction selects (host only, no context), the mapping above: *x, *y, and *jac = (l2 sqrtf(l2)) / 4, the
 * factor from pdf_st to pdf_omega there.  RT_E_ARG for a size < 1 or a NULL pointer. */
int rt_env_texel(int width, int height, const float* world_to_env, const float* dir, int* x, int* y, float* jac);
/* The bound map's device tables: *w, *h always; coeffs4 (4 w h: c0, c1, c2, m per texel), cond (w h), marg (h) when
 * non-NULL; *total = the grand total of the weights.  RT_E_STATE without a map. */
int rt_debug_env_table(rt_ctx* ctx, int* w, int* h, float* coeffs4, float* cond, float* marg, float* total);
/* The path kernels' own device functions, one item per thread: sample u (2n) -> wi (3n), pdf (n: pdf_omega), texel (n:
 * y w + x); eval dir (3n) -> texel (n), pdf (n). */
int rt_debug_env_sample(rt_ctx* ctx, int n, const float* u, float* wi, float* pdf, int32_t* texel);
int rt_debug_env_eval(rt_ctx* ctx, int n, const float* dir, int32_t* texel, float* pdf);
/* Debug only (an addition to the entry points above; rt_stats keeps its layout): *ms_miss = the miss stage's HIP-event
 * time in ms since the last rt_reset_stats (rt_stats.ms_shade includes it; 0 with RTMI_NO_STAGE_EVENTS); launches, when
 * non-NULL, 6 counts since the process started: launches of k_path_shade_full without tabled lights, with mesh lights
 * (TL = 1), with the environment (TL = 2), then the same three for k_path_nee. */
int rt_debug_env_stats(rt_ctx* ctx, double* ms_miss, int64_t* launches);

/* ---- rough reflector (additive): RT_MAT_ROUGH above ------------------------------------
 * The material's own functions on n local-frame vector pairs (host only, no context, like rt_env_texel): wo, wi 3n
 * floats each.  eval: fcos[i] = f mu_i / R = (D G2) / (4 mu_o) and pdf[i] = pdf(wo, wi), both 0 when wo.z <= 0 or
 * wi.z <= 0.  sample: disk 2n floats, the disk point (dx, dy); wi (3n), wb (n), pdf (n), all 0 where there is no bounce.
 * RT_E_ARG: a NULL pointer with n > 0, n < 0, alpha not in [0.01, 1]. */
int rt_ggx_eval(float alpha, int n, const float* wo, const float* wi, float* fcos, float* pdf);
int rt_ggx_sample(float alpha, int n, const float* wo, const float* disk, float* wi, float* wb, float* pdf);
/* The path kernels' own device functions, one item per thread, on world-space vectors: normal (3n) the shading-side
 * normal (unit), dir (3n) the incoming ray's unit direction (wo = -dir), the frame built as the shade kernel builds it.
 * sample: u (2n) the bounce's Get2D -> disk_out (2n) the disk point used, wi (3n, world space), wb, pdf (n).
 * eval: wi (3n, world space) -> fcos, pdf (n). */
int rt_debug_ggx_sample(rt_ctx* ctx, float alpha, int n, const float* normal, const float* dir, const float* u,
                        float* disk_out, float* wi, float* wb, float* pdf);
int rt_debug_ggx_eval(rt_ctx* ctx, float alpha, int n, const float* normal, const float* dir, const float* wi,
                      float* fcos, float* pdf);
/* launches[2]: launches of the RGH instantiations of k_path_shade_full and of k_path_nee (the fallback included) by the
 * context's last path pass (0, 0 for a scene without a rough material). */
int rt_debug_rough_stats(rt_ctx* ctx, int64_t* launches);

/* ---- rough glass (additive): RT_MAT_ROUGH_DIELECTRIC above --------------------------------------
 * rt_roughglass_eval / rt_roughglass_sample (host only, no context): the header's functions on vectors local to the
 * shading frame.  eval: wo, wi (3n each) -> fcosF, pdfF (n).  sample: wo (3n), disk points (2n), u (n) -> wi (3n), the
 * weight w (n, the 1 / eta_r^2 in it when transmitted), prevPdf (n) and branch (n): 0 none, 1 reflected, 2 transmitted.
 * eta_r is the relative index of the shading side (eta on the front side, 1 / eta on the back).  RT_E_ARG: alpha outside
 * [0.01, 1], eta_r not finite and positive, a negative count, a NULL pointer with a positive count. */
int rt_roughglass_eval(float alpha, float eta_r, int n, const float* wo, const float* wi, float* fcos, float* pdf);
int rt_roughglass_sample(float alpha, float eta_r, int n, const float* wo, const float* disk, const float* u, float* wi,
                         float* w, float* pdf, int32_t* branch);
/* The path kernels' own device functions at a rough-glass vertex, one item per thread, on world-space vectors as
 * rt_debug_ggx_sample / rt_debug_ggx_eval: normal (the shading-side normal), dir (the incoming ray) (3n each);
 * sample: u (3n: the bounce's Get2D, then its Get1D) -> disk_out (2n), wi (3n, world), w, pdf, branch (n);
 * eval: wi (3n, world) -> fcos, pdf (n). */
int rt_debug_roughglass_sample(rt_ctx* ctx, float alpha, float eta_r, int n, const float* normal, const float* dir,
                               const float* u, float* disk_out, float* wi, float* w, float* pdf, int32_t* branch);
int rt_debug_roughglass_eval(rt_ctx* ctx, float alpha, float eta_r, int n, const float* normal, const float* dir,
                             const float* wi, float* fcos, float* pdf);
/* launches[2]: launches of the level-3 (rough, conductor and rough glass) instantiations of k_path_shade_full and of
 * k_path_nee (the fallback included) by the context's last path pass (0, 0 for a scene without a rough glass).  On such
 * a pass rt_debug_rough_stats counts the same launches (level 3 is an RGH level), and rt_debug_conductor_stats counts
 * them only when the scene also holds a conductor. */
int rt_debug_roughglass_stats(rt_ctx* ctx, int64_t* launches);

/* ---- absorbing media inside glass (additive; build-defined: the reference has no media) ----------
 * A medium belongs to a material of type RT_MAT_DIELECTRIC or RT_MAT_ROUGH_DIELECTRIC.  Its absorption coefficient is
 * sigma_a(lambda) = sigma S(lambda), S the RGBSigmoidPolynomial of `sigmoid` as a material's R(lambda), sigma >= 0 per
 * render-space unit length.
 * The back-face rule: a path segment is attenuated when it ends on the back face of a non-emissive surface whose material
 * carries a medium with sigma > 0 (the back face by the shade kernel's own test: the ray runs along the geometric
 * normal of the triangle, or along the analytic shape's object-space normal).  Such a segment is taken to have run inside
 * the medium over its whole length len = t sqrtf((dx dx + dy dy) + dz dz), t the hit distance along the ray's
 * unnormalised direction d, and for each of the path's eight wavelengths
 *   x = (sigma S(lambda)) len;   a = x >= 87 ? 0 : (float)exp(-(double)x);   beta = beta a
 * (float32 in the order written; S with sigmoid_eval's two fmaf; terminated secondaries included).  The rule needs no
 * per-path "current medium" and is exact for closed, non-nested solids with nothing embedded in them.  The attenuation is
 * applied before the vertex is shaded, so the vertex's own light terms (a rough glass hit from inside runs NEE for its
 * reflection lobe) carry it.
 * Limits: the first segment of a camera ray is never attenuated (a camera inside a solid sees it unattenuated); a segment
 * that ends on anything else inside the solid (an embedded emitter or diffuse object) is not attenuated; no scattering;
 * shadow rays still stop at glass; RT_INTEGRATOR_REFERENCE, the feature, position, chain and albedo passes ignore media.
 *
 * rt_scene_set_media: one entry per material of the uploaded scene.  NULL or n_materials == 0 clears the media, and so
 * does rt_scene_upload (as for textures).  With no medium bound, or every sigma == 0, no pass launches anything new and
 * every film keeps its bits.  RT_E_STATE: no scene, an adaptive or temporal session is open, a multi-device context.
 * RT_E_ARG: n_materials differs from the scene's; a sigma is NaN, infinite or negative; a coefficient is not finite
 * while sigma > 0; sigma > 0 on a material whose type is not 2 or 5, or that is emissive; rt_last_error names the
 * material index and the field.  After a refusal the media bound before stay bound.
 * rt_medium_transmittance (host only, no context) and rt_debug_medium_eval (the device function the stage calls, one item
 * per thread): item j of n uses medium m[j], lambda[8j .. 8j+7] and len[j] and writes the a above to out[8j .. 8j+7].
 * RT_E_ARG: a negative count, a NULL pointer with a positive count.
 * rt_debug_medium_stats: launches of the absorb stage and the segments it attenuated in the context's last path pass
 * (0, 0 without a medium). */
typedef struct { float sigmoid[3]; float sigma; } rt_medium;
int rt_scene_set_media(rt_ctx* ctx, const rt_medium* media, int n_materials);
int rt_medium_transmittance(const rt_medium* m, int n, const float* lambda, const float* len, float* out);
int rt_debug_medium_eval(rt_ctx* ctx, const rt_medium* m, int n, const float* lambda, const float* len, float* out);
int rt_debug_medium_stats(rt_ctx* ctx, int* launches, unsigned long long* segments);

/* ---- metal (additive): RT_MAT_CONDUCTOR above ------------------------------------------
 * rt_metal_nk (host only, no context): the dense table's entry of metal (RT_METAL_*) at the dense spectra's index of
 * each of n wavelengths, n_out[i] = n, k_out[i] = k; 0 outside 360-830 nm.  rt_fresnel_conductor (host only): F[i] of
 * count (cos, n, k) triples, cos clamped to [0, 1].  RT_E_ARG: a NULL pointer with a positive count, a negative count,
 * metal out of range. */
int rt_metal_nk(int metal, int n, const float* lambda, float* n_out, float* k_out);
int rt_fresnel_conductor(int count, const float* cos, const float* n, const float* k, float* F);
/* The path kernels' own device functions for a light's wi at a conductor vertex, one item per thread, on world-space
 * vectors as rt_debug_ggx_eval (whose bits fcos and pdf have): normal, dir, wi (3n each), lambda (n) ->
 * fcos, pdf, F (n): F = F(lambda, wo.h) from the context's table.  RT_E_ARG as rt_debug_ggx_eval, and for a metal out of
 * range. */
int rt_debug_conductor_eval(rt_ctx* ctx, int metal, float alpha, int n, const float* normal, const float* dir,
                            const float* wi, const float* lambda, float* fcos, float* pdf, float* F);
/* launches[2]: launches of the level-2 (rough and conductor) instantiations of k_path_shade_full and of k_path_nee (the
 * fallback included) by the context's last path pass (0, 0 for a scene without a conductor). */
int rt_debug_conductor_stats(rt_ctx* ctx, int64_t* launches);

/* ---- albedo demodulation for the denoiser (additive) ------------------------------
 * The filter divides the film by a noise-free first-hit albedo, filters the demodulated irradiance (smooth across the
 * edges of an albedo texture) and multiplies the albedo back.  All arithmetic is float32 in the order written, unfused,
 * with only + - * /, sqrtf and fmaxf, as rt_denoise's (build-defined; tests/albedo_reference.py restates it).
 *
 * The albedo lives in the film's channel space, sensor RGB.  Every emitter is a multiple of D65, so a Lambert surface
 * of reflectance R scales channel c of directly lit radiance by
 *   A_c = sum_k (bar_c[k] D65[k]) R(360 + k) / sum_k bar_c[k] D65[k],   k = 0..470 ascending, both sums from 0,
 * bar_c the current film's sensor curves, R(l) = 0.5f + x / (2 sqrtf(1 + x x)), x = (l c0 + c1) l + c2 (1 or 0 by
 * the sign of an infinite x).  The context keeps A of every material and every texel of the scene in a lazily built
 * table (16 B per entry; rebuilt on first use after rt_scene_upload, rt_scene_set_textures or rt_film_set; a context
 * that never asks for albedo bakes nothing). */
typedef struct { float r, g, b, hits; } rt_albedo;        /* 16 B, sums over the pass's hits */
/* rt_render_features_chain that also accumulates (+=) the albedo film albedo_inout (res_x*res_y, host memory);
 * feat_inout and pos_inout (may be NULL) come out exactly as rt_render_features_chain leaves them.  The albedo is
 * always the FIRST hit's, at any chain_depth.  Per sample, in increasing index order: a miss adds nothing; under
 * RT_INTEGRATOR_REFERENCE (no material is consulted) a hit adds (1, 1, 1, 1); otherwise the hit's material is the
 * triangle's, or the analytic shape's (no texture lookup), and an emitter, a mirror or a dielectric adds (1, 1, 1, 1)
 * (emitters and specular surfaces are not demodulated); any other hit adds (A.r, A.g, A.b, 1) with A of the texel that
 * the hit's barycentrics select when the material has a texture, else of the material.
 * Work list, shards, rt_stats, error codes and multi-device contexts as rt_render_features. */
int rt_render_features_albedo(rt_ctx* ctx, int index_begin, int index_end, int chain_depth, rt_feature* feat_inout,
                              rt_position* pos_inout, rt_albedo* albedo_inout);
/* rt_denoise with demodulation by the albedo film `albedo` (res_x*res_y, host memory).  Per pixel, h = albedo.hits:
 *   a_c = h > 0 ? fmaxf(albedo_c / h, albedo_floor) : 1;   c = (film.rgb / n) / a;   sa = ((a.r + a.g) + a.b) / 3.f;
 *   var = var / (sa sa)   (var as rt_denoise computes it);  guides and depth gradient as rt_denoise;
 * rt_denoise's iterations, untouched, on (c, var); then
 *   out = ((c'.r a.r) n, (c'.g a.g) n, (c'.b a.b) n, n),   variance_out = var' (sa sa).
 * An albedo film of all (k, k, k, k) gives rt_denoise's bits.  albedo_floor must be finite and in (0, 1] (RT_E_ARG
 * otherwise); NULL and overlap rules as rt_denoise, with albedo an input. */
int rt_denoise_albedo(rt_ctx* ctx, const rt_denoise_desc* desc, float albedo_floor, int res_x, int res_y,
                      const rt_pixel* film, const rt_moment* mom, const rt_feature* feat, const rt_albedo* albedo,
                      rt_pixel* out, float* variance_out);
/* rt_adaptive_denoise with a session-owned device albedo film of indices [0, feature_samples), rendered with the
 * features once per session (again when feature_samples or chain_depth change).  The session's film, moments and
 * active list are untouched.  rt_adaptive_denoise itself neither renders nor allocates an albedo film.
 * Multi-device contexts: RT_E_STATE, as the feature pass. */
int rt_adaptive_denoise_albedo(rt_ctx* ctx, const rt_denoise_desc* desc, float albedo_floor, rt_pixel* film_out);
/* The bake kernel alone: n coefficient triples (3n floats) -> 3n floats (A_r, A_g, A_b) under the current film's
 * sensor (the XYZ sensor until rt_film_set). */
int rt_debug_albedo_bake(rt_ctx* ctx, int n, const float* coeffs, float* rgb);

/* ---- instrumentation ---------------------------------------------------------------------------- */
int rt_get_stats(rt_ctx* ctx, rt_stats* out);
int rt_reset_stats(rt_ctx* ctx);
int rt_octree_get_info(rt_ctx* ctx, rt_octree_info* out);
/* Copy out the flattened octree: node_bounds[6*n] (pmin,pmax), node_child[n] (first child or -1),
 * node_leaf_first[n], node_leaf_count[n], leaf_refs[n_leaf_refs] (triangle ids incl. culled ones). */
int rt_octree_export(rt_ctx* ctx, float* node_bounds, int32_t* node_child, int32_t* node_leaf_first,
                     int32_t* node_leaf_count, int32_t* leaf_refs);
/* The fast multi-level traversal's 8-wide compressed BVH as uploaded: set 0 / 1 the closest-hit BVH of tile set 0 (all
 * triangles) / 1 (without back faces), set 2 the any-hit BVH of the shadow rays (all triangles), DESIGN.md §6b: *n_nodes nodes of 32 floats (128 B, layout in rt_bvh.cpp), *n_tiles triangle tiles of
 * 12 floats, consts[2] = (wabs, oguard) of the canonical rule.  Counts always; arrays when non-NULL.  Not a
 * reference structure (the reference traverses only its octree): exported so tests can replay the GPU's walk. */
int rt_bvh_export(rt_ctx* ctx, int set, int* n_nodes, int* n_tiles, float* consts, float* nodes, float* tiles);
/* The same BVH built on the host from a scene descriptor, without a context or a device (CPU tests). */
int rt_debug_bvh_build(const rt_scene_desc* scene, int set, int* n_nodes, int* n_tiles, float* consts, float* nodes,
                       float* tiles);

/* ---- parity entry points (same kernels as the hot path, stage outputs exposed) ------------------ */
/* K2 alone: closest hit of n world-space rays (ro, rd: 3n floats).  prim[n] (-1 = miss),
 * bt[4n] = (b0, b1, b2, t).  use_cull follows the reference's back-face flags. */
int rt_debug_trace(rt_ctx* ctx, int n, const float* ro, const float* rd, int use_cull, int32_t* prim, float* bt);
/* The path integrator's shadow query alone: any hit of n rays within (0, tmax[i]) against the octree and the
 * analytic shapes (Octtree_Model.h:66-127 with the early exit, Shapes.h shape tests); occluded[n] = 0 / 1. */
int rt_debug_occluded(rt_ctx* ctx, int n, const float* ro, const float* rd, const float* tmax, int32_t* occluded);
/* K1..K3 for n explicit (pixel_id, index) samples (reference integrator). */
int rt_debug_samples(rt_ctx* ctx, int n, const int32_t* pixel_ids, const int32_t* indices, rt_sample_record* out);
/* The multi-level coherence sorts alone (rt_sort.hip: stable device LSD radix sorts) on a synthetic queue of
 * RT_QUEUE_SHARDS shards of stride S (a multiple of 64): shard j holds shard_len[j] <= S items at positions
 * [j S, j S + shard_len[j]), with keys[pos] (8 S entries) and, for the NEE sort, slots[pos].  which 0: the bounce-ray
 * sort (key bits 3 + 2 bits_a + 3 bits_b; out[pos'] = the queue position of the sorted item at pos'); which 1: the
 * NEE-vertex sort (key bits 3 bits_a; out = the slots, sorted in place).  Sorted item k' sits at position
 * (k' / S2) S + k' % S2, S2 = ceil(ceil(n / 8) / 64) 64; out_len[8] = the rewritten shard lengths.  Not a
 * reference function (the reference has no sort): exported so tests can check order and stability directly. */
int rt_debug_sort(rt_ctx* ctx, int which, int S, const int32_t* shard_len, const uint32_t* keys, const int32_t* slots,
                  int bits_a, int bits_b, int32_t* out, int32_t* out_len);

#ifdef __cplusplus
}
#endif
#endif /* RTMI355X_H */
