/*
 * tvam.h — C ABI of the MI355X-native TVAM projection engine (libtvam.so).
 *
 * This is the drop-in boundary for Dr.TVAM's hot path: the per-angle voxel-grid
 * ray march behind the `volume` integrator + `dda` sensor + `vfilm` film +
 * `collimated` / `telecentric` / `lens` projector plugins.  Every entry point names the reference
 * interface it replaces (paths relative to the drtvam source tree):
 *
 *   tvam_plan_create   <- scene assembly: optimize.py:15-79 (load_scene),
 *                         TVAMProjector.__init__ projector.py:41-139,
 *                         CollimatedProjector.__init__ projector.py:167-182,
 *                         TelecentricProjector / LensProjector.__init__ projector.py:199-271,
 *                         CircularMotion motion.py:19-36,
 *                         VolumetricSensor.__init__ sensor.py:5-22,
 *                         VolumetricFilm.__init__ film.py:4-21,
 *                         IndexMatchedVial.to_dict geometry.py:75-96,
 *                         TVAMIntegrator.__init__ integrators/common.py:6-22
 *   tvam_forward       <- VolumeIntegrator.render integrators/volume.py:18-56
 *                         (+ sample() :136-282, DDAVolumetricSensor.accumulate
 *                         sensor.py:306-440 primal branch, VolumetricFilm.write
 *                         film.py:40-41)
 *   tvam_adjoint       <- VolumeIntegrator.render_backward integrators/volume.py:97-134
 *                         (+ accumulate backward branch sensor.py:417-423 and
 *                         dr.backward_from(Le * em_grad) volume.py:274-276)
 *   tvam_forward_dsigma, tvam_adjoint_dsigma <- the medium derivative of the same march: the
 *                         sigma_t tangent of render_forward (volume.py:58-95, sensor.py:371-375) and
 *                         st_grad of accumulate sent into sigma_t (sensor.py:377-440, volume.py:274-280)
 *   tvam_count_visits  <- (new) exact DDA visit count H used for the roofline
 *   tvam_loss_threshold<- ThresholdedLoss.__call__ loss.py:28-59, :119-132 (fused
 *                         value + dL/dx, also used for the Armijo probes of
 *                         LinearLBFGS.step lbfgs.py:256-266)
 *   tvam_loss_threshold_probes <- the same Armijo probes, up to 8 step sizes per pass
 *                         (lbfgs.py:255-268: one loss pass and one host read per batch)
 *   tvam_loss_square, tvam_loss_surface (+ _probes) <- L2Loss.__call__ loss.py:62-79 and both
 *                         losses over a surface-aware target, loss.py:39-47 (fused the same way)
 *   tvam_plan_destroy, tvam_last_error  <- Python exception plumbing
 *
 * All buffers are caller-owned device pointers (e.g. torch tensors' data_ptr()).
 * Calls are asynchronous on the given HIP stream; a plan is bound to one device
 * and is not thread-safe.  Functions return 0 on success and a negative
 * TVAM_ERR_* code on failure; tvam_last_error() then returns a thread-local
 * message (the Python shim re-raises it with the reference's wording).
 */
#ifndef TVAM_H_
#define TVAM_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TVAM_ABI_VERSION 13

/* error codes */
#define TVAM_OK               0
#define TVAM_ERR_INVALID     -1   /* bad descriptor / argument (ValueError)  */
#define TVAM_ERR_UNSUPPORTED -2   /* configuration not implemented yet        */
#define TVAM_ERR_HIP         -3   /* HIP runtime failure (RuntimeError)      */
#define TVAM_ERR_TOO_LARGE   -4   /* > 2^32 samples, common.py:60-65          */

/* projector kinds (projector.py:300-302) */
#define TVAM_PROJECTOR_COLLIMATED 0
#define TVAM_PROJECTOR_TELECENTRIC 1  /* projector.py:199-237: parallel chief rays, finite aperture */
#define TVAM_PROJECTOR_LENS        2  /* projector.py:241-296: thin lens, chief rays through the lens centre */
/* vial / container kinds (geometry.py:312-318) */
#define TVAM_VIAL_INDEX_MATCHED   0
#define TVAM_VIAL_CYLINDRICAL     1
#define TVAM_VIAL_SQUARE          2  /* glass cuboids w_ext / w_int (vial_r = w_int/2, vial_r_ext = w_ext/2) */
#define TVAM_VIAL_CUSTOM          3  /* dielectric triangle meshes (tvam_plan_create_mesh; vial_r, vial_r_ext and
                                        vial_height unused) */
#define TVAM_VIAL_DOUBLE_CYLINDRICAL 4  /* two nested glass tubes (tvam_plan_create_double; vial_r and vial_r_ext
                                        unused: the radii are tvam_double_vial's) */

/* medium phase functions (Mitsuba 'isotropic', 'rayleigh', 'hg'; geometry.py:29-39) */
#define TVAM_PHASE_ISOTROPIC      0
#define TVAM_PHASE_RAYLEIGH       1
#define TVAM_PHASE_HG             2
/* sensor kinds (sensor.py:442-444) */
#define TVAM_SENSOR_DDA           0  /* analytic absorption per voxel visit (sensor.py:297-440) */
#define TVAM_SENSOR_RATIO         1  /* ratio tracking at a majorant (sensor.py:193-295) */
#define TVAM_SENSOR_DELTA         2  /* collision estimator at the medium interactions (sensor.py:112-191) */

/*
 * Scene + integrator description.  Plain old data; every field mirrors a
 * reference property of the same meaning.
 */
typedef struct tvam_desc {
    int32_t abi_version;          /* must be TVAM_ABI_VERSION */

    /* projector: TVAMProjector props (projector.py:73-99) */
    int32_t projector_type;       /* TVAM_PROJECTOR_* */
    int32_t n_patterns;           /* 'n_patterns' (A) */
    int32_t res_x, res_y;         /* 'resx', 'resy' (full DMD W, H) */
    int32_t crop_x, crop_y;       /* 'cropx', 'cropy' */
    int32_t crop_offset_x, crop_offset_y; /* 'crop_offset_x/_y' */
    float   pixel_size_x, pixel_size_y;   /* 'pixel_size' (projector.py:171-175) */

    /* motion: CircularMotion (motion.py:19-24) */
    float   distance;             /* 'distance' */
    int32_t clockwise;            /* 'clockwise' */

    /* sensor + film: bbox = to_world @ [-0.5,0.5]^3 (sensor.py:14-16);
       film resolution in film order: res.x = props['resy'],
       res.y = props['resx'], res.z = props['resz'] (film.py:9-14) */
    int32_t sensor_type;          /* TVAM_SENSOR_* */
    float   bbox_min[3], bbox_max[3];
    int32_t film_res[3];
    int32_t film_channels;        /* 1, or 2 = 'surface_aware' (film.py:16-21): channel 0 collects
                                     the segments inside the target mesh, 1 those outside
                                     (sensor.py:405-409); needs target_tris */

    /* container (geometry.py:20-35, :75-96, :142-183) */
    int32_t vial_type;            /* TVAM_VIAL_* */
    float   vial_r;               /* index_matched 'r' (or cylindrical 'r_int') */
    float   vial_r_ext;           /* cylindrical 'r_ext' */
    float   vial_height;          /* 'height' (default 40) */
    float   vial_ior;             /* cylindrical 'ior' */
    float   medium_ior;           /* medium 'ior' */
    float   sigma_t;              /* medium 'extinction' */
    float   albedo;               /* medium 'albedo' */

    /* integrator props (integrators/common.py:6-22, optimize.py:96-128) */
    float   print_time;           /* 'print_time' (config 'time') */
    int32_t regular_sampling;     /* 'regular_sampling' */
    int32_t sample_time;          /* 'sample_time' */
    int32_t max_depth;            /* 'max_depth' */
    int32_t rr_depth;             /* 'rr_depth' */
    int32_t transmission_only;    /* 'transmission_only' */

    /* execution (new): angle shard [angle_begin, angle_end) of this rank and
       the LDS tile edge in voxels (0 = auto) */
    int32_t angle_begin, angle_end;
    int32_t tile;
    int32_t flags;                /* TVAM_FLAG_* */
    /* film slab [slab_begin, slab_end) of z-slices this plan renders (-1 =
       whole film): the dose / grad_dose buffers hold only these slices, and
       rays of other slices are skipped (z-slab sharding of planar scenes) */
    int32_t slab_begin, slab_end;
    /* scattering media (albedo > 0): medium 'phase' {'type', 'g'} */
    int32_t phase_type;           /* TVAM_PHASE_* */
    float   phase_g;              /* 'hg' asymmetry g */
    /* occluder meshes ('occlusions', geometry.py:55-72): black diffuse
       triangles; host array [n_occluder_tris][3 vertices][x, y, z], read by
       tvam_plan_create (not kept) */
    const float* occluder_tris;
    int32_t n_occluder_tris;
    /* target mesh (optimize.py:64-73: null BSDF, kept in the scene when the
       film is surface-aware, optimize.py:188-191): host array
       [n_target_tris][3 vertices][x, y, z] in world space, read by
       tvam_plan_create (not kept).  Used when film_channels == 2. */
    const float* target_tris;
    int32_t n_target_tris;
    /* 'ratio' sensor: its 'majorant' (sensor.py:195) */
    float   majorant;
    int32_t reserved0;
    /* Position of a sparse active_pixels[0] in the whole projector.active_pixels
       when the active set is split over plans (angle shards): the sampler stream of
       entry i is (active_base + i) * spp + sample, as TVAMIntegrator.prepare /
       sample_rays seed it (common.py:57-67, :81).  Dense calls (active_pixels ==
       NULL) use the global dense crop index, which is that position already. */
    int64_t active_base;
    /* len(projector.active_data) of the whole (unsharded) active set: the ray weight
       inv_pdf / n_samples = pixel area * active_total / (active_total * spp)
       (projector.py:164-165, :187) in the reference's fp32 rounding; 0 = the call's
       n_active. */
    int64_t active_total;
    /* 'telecentric' / 'lens' projectors (ABI v13; projector.py:204-205, :245-246): every ray starts
       on the aperture disk (radius aperture_radius, sampled with square_to_uniform_disk_concentric)
       and passes its pixel's point of the plane at focus_distance.  'lens': pixel_size_x =
       pixel_size_y = the pixel size at the focus plane (from 'fov' or 'pixel_size',
       projector.py:252-262).  Unused by 'collimated'. */
    float   aperture_radius;
    float   focus_distance;
} tvam_desc;

/* tvam_desc.flags */
#define TVAM_FLAG_NO_ZERO_SKIP 1  /* forward: march rays whose pattern value is 0 too */
#define TVAM_FLAG_FWD_STATS    2  /* forward: count tiles that fell back to float LDS atomics */
#define TVAM_FLAG_NO_PLANAR    4  /* use the per-ray tile kernels even where the planar path applies */
#define TVAM_FLAG_RAY_FWD      8  /* planar path: ray-driven forward instead of the voxel-driven one */
#define TVAM_FLAG_SCATTER_ATOMIC 16 /* scattering media: per-path global atomics / gathers instead of brick bins;
                                       telecentric / lens projectors: the per-ray atomic forward */
#define TVAM_FLAG_BIN_FIRST    32  /* telecentric / lens projectors: the brick-binned forward (neither flag: the
                                       plan's default forward) */

typedef struct tvam_plan tvam_plan;

/* Fill *desc with the reference defaults (scene-independent fields). */
void tvam_desc_init(tvam_desc* desc);

/* Validate desc, build per-angle / per-slice / per-tile tables on `device`. */
int  tvam_plan_create(const tvam_desc* desc, int device, tvam_plan** plan);
void tvam_plan_destroy(tvam_plan* plan);

/*
 * A plan behind a 'custom' vial (vial_type = TVAM_VIAL_CUSTOM; geometry.py:98-138): the outer
 * (air / glass, eta = vial_ior / air) and inner (glass / medium, eta = medium_ior / vial_ior)
 * surfaces are triangle meshes with dielectric interfaces and face normals
 * n = normalize((v1 - v0) x (v2 - v0)); the winding decides the side, and both meshes must be
 * wound outwards.  outer_tris / inner_tris: host arrays [n][3 vertices][x, y, z] in world space,
 * read here and not kept.  Every ray's path through the interfaces is traced in 3-D (a closest-hit
 * query against a bounding volume hierarchy built here), so such a plan runs the per-ray 3-D
 * kernels for all three projectors.  TVAM_ERR_INVALID: null or empty meshes, non-finite vertices,
 * a zero-area triangle (the message names the mesh and the triangle).  TVAM_ERR_UNSUPPORTED, by
 * name: occluders, albedo > 0, the ratio / delta sensors, a surface-aware film, film slabs,
 * transmission_only = 0, rr_depth < 2.  tvam_plan_create refuses TVAM_VIAL_CUSTOM and names this
 * entry.
 */
int tvam_plan_create_mesh(const tvam_desc* desc, const float* outer_tris, int32_t n_outer,
                          const float* inner_tris, int32_t n_inner, int device, tvam_plan** plan);

/*
 * Closest hit of n_rays rays (o, d: [n_rays][3], host) with a triangle mesh (tris: [n][3][3],
 * host), on the host with the code the kernels run: t[i] = the nearest hit distance >= 0 (+inf:
 * none) and tri[i] = its triangle (-1: none); ties in t go to the lower triangle index.
 * use_bvh = 1 builds the hierarchy a plan builds and traverses it, use_bvh = 0 loops over every
 * triangle: both return the same t (bit for bit) and tri.  No GPU is touched.
 */
int tvam_mesh_hit(const float* tris, int32_t n, const float* o, const float* d, int64_t n_rays, int32_t use_bvh,
                  float* t, int32_t* tri);

/*
 * A 'double_cylindrical' vial (geometry.py:222-308): four concentric open tubes around z with
 * |z| <= vial_height / 2 and outward normals, outermost first.  The printing medium fills the gap
 * between the outer vial's inside wall (r_int_outer) and the inner vial's outside wall
 * (r_ext_inner); the core inside r_int_inner holds no resin.  vial_height, medium_ior and sigma_t
 * are the descriptor's.
 */
typedef struct tvam_double_vial {
    float r_ext_outer;       /* air            | outer glass */
    float r_int_outer;       /* outer glass    | medium      */
    float r_ext_inner;       /* medium         | inner glass */
    float r_int_inner;       /* inner glass    | core        */
    float ior_outer;         /* outer glass */
    float ior_inner;         /* inner glass */
    float ior_inside_inner;  /* the core */
} tvam_double_vial;

/*
 * A plan behind a 'double_cylindrical' vial (vial_type = TVAM_VIAL_DOUBLE_CYLINDRICAL).  Every ray
 * is traced in 3-D through the four dielectric tubes (volume.py:179-272 in transmission-only mode:
 * nearest hit, Fresnel transmission, spawn offset, medium flag, at most max_depth surfaces) and
 * deposits along 0, 1 or 2 medium segments: before and, for rays that cross the inner vial, behind
 * it; the second segment's weight carries e^{-sigma_t t} of the first.  Such a plan runs per-ray
 * 3-D kernels for all three projectors.  TVAM_ERR_INVALID unless r_ext_outer > r_int_outer >
 * r_ext_inner > r_int_inner > 0 and all IORs are positive.  TVAM_ERR_UNSUPPORTED, by name:
 * occluders, albedo > 0, the ratio / delta sensors, a surface-aware film, film slabs,
 * transmission_only = 0, rr_depth < min(max_depth, 7) - 1 (Russian roulette would act on or before
 * a deposit).  All of it is checked before any device call.  tvam_plan_create refuses
 * TVAM_VIAL_DOUBLE_CYLINDRICAL and names this entry.
 */
int tvam_plan_create_double(const tvam_desc* desc, const tvam_double_vial* vial, int device, tvam_plan** plan);

/*
 * The medium segments of a call's rays behind a 'double_cylindrical' vial: segs is a device array
 * [n_active * spp][2][8] floats in sampler-stream order (row = active entry * spp + sample), each
 * segment o2[3], maxt, d2[3], weight (the whole per-ray weight of tvam_plan_rays times the
 * attenuation the segment starts with); a slot without a segment is all zeros.  active_pixels as
 * in tvam_forward.  TVAM_ERR_UNSUPPORTED on any other plan.  tvam_plan_rays on such a plan gives
 * the projector ray and the first segment in its own layout.
 */
int tvam_plan_segments(tvam_plan* plan, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                       uint32_t seed, float* segs, void* hip_stream);

/*
 * The same segments on the host, with the code the kernels run and no GPU touched: n_rays world
 * rays (o, d: [n_rays][3], host) through `vial`, segs: host [n_rays][2][8] in the layout above with
 * weight = the attenuation alone.  TVAM_ERR_INVALID for a vial tvam_plan_create_double refuses.
 */
int tvam_double_segments(const tvam_double_vial* vial, float medium_ior, float sigma_t, float height,
                         int32_t max_depth, const float* o, const float* d, int64_t n_rays, float* segs);

/*
 * A plan behind a 'cylindrical' or 'square' glass vial whose rays are traced in 3-D (vial_type =
 * TVAM_VIAL_CYLINDRICAL or TVAM_VIAL_SQUARE, any projector kind): the entry for the telecentric and
 * lens projectors behind a glass tube or cuvette, which tvam_plan_create refuses, naming this one.
 * Every ray is traced through the two analytic dielectric surfaces (volume.py:179-272 in
 * transmission-only mode: nearest hit of the outer and the inner surface, a tie to the inner one,
 * Fresnel transmission, spawn offset, medium flag, at most max_depth surfaces) to its one medium
 * segment, and the plan runs the per-ray 3-D kernels.  cylindrical: open tubes of radius vial_r_ext
 * and vial_r with |z| <= vial_height / 2 and no end caps, so a ray may enter or leave through an open
 * end (one that leaves the medium that way deposits nothing); square: closed cuboids of half width
 * vial_r_ext and vial_r, the inner one 0.9 of the height, all six faces.  A collimated descriptor
 * through this entry runs the same 3-D path (tvam_plan_create gives it the planar kernels).
 * TVAM_ERR_UNSUPPORTED, as "the '<kind>' projector with <what>": occluders, albedo > 0, the ratio /
 * delta sensors, a surface-aware film, film slabs, transmission_only = 0, rr_depth < 2.
 * TVAM_ERR_INVALID: any other vial type, r_ext <= r_int, non-positive radii / height / IORs, a bad
 * focus_distance / aperture_radius.  All of it is checked before any device call.  On such a plan
 * tvam_plan_rays gives d2 in [11:14] and weight x the interfaces' transmission in [14]; tvam_radon
 * refuses it; tvam_corner serves it.
 */
int tvam_plan_create_traced(const tvam_desc* desc, int device, tvam_plan** plan);

/*
 * The medium segments of such a plan's tracer on the host, with the code the kernels run and no GPU
 * touched: n_rays world rays (o, d: [n_rays][3], host), segs: host [n_rays][8] = o2[3], maxt, d2[3],
 * att (the interfaces' transmission weight); a row is all zeros when the ray deposits nothing.
 * TVAM_ERR_INVALID for a descriptor tvam_plan_create_traced would refuse.
 */
int tvam_traced_segments(const tvam_desc* desc, const float* o, const float* d, int64_t n_rays, float* segs);

/*
 * A dielectric occluder (geometry.py:55-72 with a 'bsdf' entry of type 'dielectric'): a transparent
 * insert inside the resin, the overprinting case.  tris: host [n_tris][3][3], a closed mesh wound
 * outwards (face normal normalize((v1 - v0) x (v2 - v0))); int_ior / ext_ior: the BSDF's own numbers
 * (eta = int_ior / ext_ior whatever the resin's IOR is).  The insert's exterior is the printing
 * medium and it has no interior medium: a ray refracts into it, crosses it without dose or
 * attenuation, refracts out and goes on depositing.
 */
typedef struct tvam_insert {
    const float* tris;
    int32_t n_tris;
    float int_ior;
    float ext_ior;
} tvam_insert;

/*
 * A plan whose resin holds dielectric occluders, behind an 'index_matched', 'cylindrical' or
 * 'square' vial (the last two as tvam_plan_create_traced describes them) with any of the three
 * projectors.  Every ray runs the path loop of volume.py:179-272 in transmission-only mode: per
 * iteration one Russian roulette draw (it acts when depth > rr_depth, q = min(0.99, attenuation)),
 * the nearest hit over the container's surfaces, then the descriptor's black occluders, then the
 * insert triangles (a later candidate wins only when strictly nearer; none: the path ends and a
 * segment in progress deposits nothing), a medium segment up to the hit when the ray is in the
 * resin, then: a black occluder ends the path; any other surface multiplies the attenuation by its
 * Fresnel transmission (0, total internal reflection, ends the path) and, after a medium segment,
 * by e^{-sigma_t t}; the medium flag is on behind the container's medium boundary crossed inwards
 * and behind an insert face crossed outwards, off otherwise.  At most max_depth surfaces.  A ray so
 * deposits along any number of segments, which may leave their z-plane: the plan runs per-ray 3-D
 * kernels (forward: float atomics; adjoint: a gather).  The triangles are read here and not kept.
 * TVAM_ERR_INVALID, naming the insert and the triangle or vertex: null or empty meshes, non-finite
 * vertices, zero-area triangles, non-positive IORs, a vertex outside the resin (tubes: radius >=
 * vial_r or |z| > vial_height / 2; square: outside the inner cuboid).  TVAM_ERR_UNSUPPORTED, as
 * "dielectric occluders with <what>": albedo > 0, the ratio / delta sensors, a surface-aware film,
 * film slabs, transmission_only = 0, a 'custom' or 'double_cylindrical' vial.  All of it is checked
 * before any device call.  On such a plan tvam_plan_rays gives the projector ray and the first
 * segment in the traced plans' layout, tvam_corner and tvam_count_visits serve it, and tvam_radon,
 * tvam_forward_dsigma, tvam_adjoint_dsigma, tvam_forward_slices, tvam_adjoint_slices and
 * tvam_plan_segments refuse it by name.
 */
int tvam_plan_create_inserts(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts, int device,
                             tvam_plan** plan);

/*
 * The medium segments of that walk on the host, with the code the kernels run and no GPU touched:
 * n_rays world rays (o, d: [n_rays][3], host); u: [n_rays][max_depth][4] host, the four draws of
 * each loop iteration (roulette, then the BSDF's three, ignored), or NULL: roulette never acts.
 * segs: host [n_rays][max_segments][8], each segment o2[3], maxt, d2[3], weight = the attenuation
 * the segment starts with, zeros past the ray's segments; nseg: host [n_rays], the segments the ray
 * has (beyond max_segments they are counted and not written).  TVAM_ERR_INVALID /
 * TVAM_ERR_UNSUPPORTED as tvam_plan_create_inserts.
 */
int tvam_insert_segments(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts, const float* o,
                         const float* d, int64_t n_rays, const float* u, int32_t max_segments, float* segs,
                         int32_t* nseg);

/*
 * The same on the device for a call's rays: segs [n_active * spp][max_segments][8] floats (16-byte
 * aligned) and nseg [n_active * spp] in sampler-stream order as tvam_plan_segments defines it, the
 * weight as there (the whole per-ray weight times the attenuation the segment starts with).
 * TVAM_ERR_UNSUPPORTED on a plan that neither tvam_plan_create_inserts nor tvam_plan_create_reflect
 * made.
 */
int tvam_plan_insert_segments(tvam_plan* plan, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                              uint32_t seed, int32_t max_segments, float* segs, int32_t* nseg, void* hip_stream);

/*
 * Reflected paths: a plan for transmission_only = 0 (common.py:19; every other entry refuses that
 * value behind a refracting container).  The walk is tvam_plan_create_inserts' with the BSDF's
 * first draw used: at a path's first surface the transmission is forced as there, weight
 * (1 - F) eta_ti^2; at every later dielectric surface (the vial's outer and inner glass, an insert
 * face) the iteration's second draw s1 is compared with the Fresnel reflectance F: s1 <= F reflects
 * (wo = d - 2 (d . n) n, weight 1), otherwise the ray refracts with weight eta_ti^2.  Total internal
 * reflection (F = 1) therefore reflects and no longer ends the path.  The index-matched tube still
 * passes the ray on and a black occluder still ends it.  After either branch: e^{-sigma_t t} after a
 * medium segment, the spawn offset on the side of wo, the medium flag (container's medium boundary
 * and n . wo < 0, or insert face and n . wo > 0: a reflection off the inner wall from the resin
 * stays in the resin and starts a new segment), ++depth.  Such a walk draws its four numbers in
 * every iteration, whether or not Russian roulette can act.
 * Accepted: 'cylindrical' and 'square' vials with n_inserts >= 0, 'index_matched' with
 * n_inserts >= 1, the three projectors, black occluders, crop, clockwise, regular and jittered
 * sampling, sample_time, dense and sparse sets, angle shards, any max_depth / rr_depth.
 * TVAM_ERR_INVALID: transmission_only = 1 (that mode is the other entries'), an index-matched vial
 * without inserts, and tvam_plan_create_inserts' mesh checks.  TVAM_ERR_UNSUPPORTED, as
 * "transmission_only = 0 with <what>": albedo > 0, the ratio / delta sensors, a surface-aware film,
 * film slabs, a 'custom' or 'double_cylindrical' vial.  All before any device call.  tvam_forward,
 * tvam_adjoint, tvam_corner, tvam_count_visits, tvam_plan_rays and tvam_plan_insert_segments serve
 * such a plan; tvam_radon, the dsigma and dprojector entries, the slice entries and
 * tvam_plan_segments refuse it by name.
 */
int tvam_plan_create_reflect(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts, int device,
                             tvam_plan** plan);

/*
 * That walk on the host, as tvam_insert_segments; u ([n_rays][max_depth][4]: roulette, s1, and the
 * two of s2, unused) is required.
 */
int tvam_reflect_segments(const tvam_desc* desc, const tvam_insert* inserts, int32_t n_inserts, const float* o,
                          const float* d, int64_t n_rays, const float* u, int32_t max_segments, float* segs,
                          int32_t* nseg);

/*
 * Forward projection (primal render).  Writes the whole film
 * dose[z][y][x][C] (film order) = inv_vol * sum over rays of this plan's
 * angle shard; every voxel is overwritten (no pre-zeroing needed).
 *   active_data   : f32, n_active entries (projector.active_data)
 *   active_pixels : u32 flat indices angle*H*W + row*W + col into the full DMD
 *                   (projector.active_pixels); NULL means the dense crop order
 *                   produced by TVAMProjector.__init__ (projector.py:90-98),
 *                   in which case n_active must equal A*crop_y*crop_x.
 *                   Jittered sampling: the plan keeps the per-ray records of a sparse set
 *                   keyed on (active_pixels pointer, n_active, seed, spp) and reuses them
 *                   (slice ranges, the line-search forward of one seed); after changing the
 *                   array's contents in place, or before passing a different array (a new
 *                   allocation can land on a freed one's address), call
 *                   tvam_plan_set_active, which drops them.
 * spp / seed follow TVAMIntegrator.prepare (common.py:41-68).
 */
int tvam_forward(tvam_plan* plan, const float* active_data,
                 const uint32_t* active_pixels, uint64_t n_active,
                 uint32_t spp, uint32_t seed, float* dose, void* hip_stream);

/*
 * Forward projection of film slices [z_begin, z_end) only (relative to the plan's slab): the
 * same values tvam_forward writes there, the other slices of dose untouched.  Lets a caller
 * all-reduce a finished slice range of an angle shard's partial dose while the next range is
 * computed.  The range must lie on the forward's slice chunks
 * (tvam_plan_fwd_chunk); TVAM_ERR_UNSUPPORTED when the plan's forward cannot be split (0).
 */
int tvam_forward_slices(tvam_plan* plan, const float* active_data,
                        const uint32_t* active_pixels, uint64_t n_active,
                        uint32_t spp, uint32_t seed, int32_t z_begin, int32_t z_end,
                        float* dose, void* hip_stream);
/* Slice granularity of tvam_forward_slices (0: the plan's forward covers every slice at once:
   scattering media, per-path kernels, the ray-driven planar forward). */
int tvam_plan_fwd_chunk(const tvam_plan* plan);

/*
 * Adjoint projection (render_backward).  grad_active[i] (overwritten, f32,
 * n_active entries) = d<grad_dose, forward(active_data)>/d active_data[i],
 * i.e. the gradient Dr.TVAM accumulates into projector.active_data.grad.
 */
int tvam_adjoint(tvam_plan* plan, const float* grad_dose,
                 const uint32_t* active_pixels, uint64_t n_active,
                 uint32_t spp, uint32_t seed, float* grad_active,
                 void* hip_stream);

/*
 * Extinction derivatives: d dose / d sigma_t of a non-scattering medium in forward and reverse mode,
 * the reference's g_st (DDAVolumetricSensor.accumulate sensor.py:377-440, sent into sigma_t by
 * volume.py:274-280; forward mode sensor.py:371-375, volume.py:58-95).  (Added to ABI v13: no struct
 * or existing signature changed.)  With albedo = 0 only the visit weight depends on sigma_t: a visit
 * that starts at in-medium path length T0 (from the segment origin) and lasts dt deposits
 * e^{-s T0} - e^{-s (T0 + dt)}, whose derivative is
 *   w'(T0, dt) = e^{-s T0} (dt (1 - q) - T0 q),  q = 1 - e^{-s dt}.
 *
 *   tvam_forward_dsigma: tangent (device, f32, the dose's layout, overwritten) = the forward render of
 *     active_data with w' in place of the visit weight: T[v] = d dose[v] / d sigma_t.
 *   tvam_adjoint_dsigma: g_sigma[0] (device, f64, overwritten) = sum_v grad_dose[v] T[v], the gradient
 *     of <grad_dose, tvam_forward(active_data)> in sigma_t.  Per ray a gather in f32, the rays summed in
 *     f64 in an order that depends on the ray count alone: no float atomics, identical calls give
 *     identical bits.
 *   active_data, active_pixels, n_active, spp, seed as in tvam_forward (angle shards, crops, sparse
 *   sets, jittered sampling with the plan's own sampler streams).  Asynchronous on hip_stream.  Both
 *   march every ray's first medium segment with the reference's DDA stepping, whichever forward the
 *   plan picked (planar, ray-driven, tile or 3-D per-ray).
 *   TVAM_ERR_UNSUPPORTED, the message starting "tvam_forward_dsigma: " / "tvam_adjoint_dsigma: " and
 *   naming the cause, checked before any device call: albedo > 0, the ratio / delta sensors, a
 *   surface-aware film, a film slab, sample_time, a 'double_cylindrical' plan.
 *   tvam_dsigma_weights: w[i] = w'(T0[i], dt[i]) at sigma_t on the host (n entries each), with the
 *     kernels' own expression in f32.  No GPU is touched.
 */
int tvam_forward_dsigma(tvam_plan* plan, const float* active_data, const uint32_t* active_pixels,
                        uint64_t n_active, uint32_t spp, uint32_t seed, float* tangent, void* hip_stream);
int tvam_adjoint_dsigma(tvam_plan* plan, const float* active_data, const float* grad_dose,
                        const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                        double* g_sigma /* device, overwritten */, void* hip_stream);
int tvam_dsigma_weights(float sigma_t, const float* T0, const float* dt, int64_t n, float* w);

/*
 * Projector derivatives: d dose / d theta for one parameter theta of a telecentric / lens projector,
 * in forward and reverse mode.  (Added to ABI v13: no struct or existing
 * signature changed.)  The derivative is pathwise: the sampler draws, the (ray, sample) -> voxel
 * bookkeeping and every discrete decision are held fixed, as are the other descriptor fields.  Every
 * visit's weight e^{-s t_a} - e^{-s t_b} moves with the times t_a, t_b at which the ray crosses the
 * voxel's faces: s (e^{-s t_b} t_b' - e^{-s t_a} t_a').  Rays that cross the tube's silhouette or its
 * open ends as theta moves (a visibility change) are not accounted for.
 *
 *   param (TVAM_DPROJ_*): 'distance'; 'focus_distance'; 'aperture_radius'; 'pixel_size' =
 *     pixel_size_x and pixel_size_y moved together (the directional derivative along (1, 1), the ray
 *     weight ~ p_x p_y included).
 *   tvam_forward_dprojector: tangent (device, f32, the dose's layout, overwritten) = T[v] =
 *     d dose[v] / d theta of tvam_forward(active_data).
 *   tvam_adjoint_dprojector: g[0] (device, f64, overwritten) = sum_v grad_dose[v] T[v].  Per ray a
 *     gather in f32, the rays summed in f64 in an order that depends on the ray count alone: no float
 *     atomics, identical calls give identical bits.
 *   active_data, active_pixels, n_active, spp, seed as in tvam_forward (angle shards, crops, sparse
 *   sets, clockwise, regular / jittered sampling, sample_time).  Asynchronous on hip_stream.
 *   Served: telecentric and lens plans of tvam_plan_create behind the index-matched vial, non-scattering
 *   medium, 'dda' sensor, one-channel film.  Every other plan: TVAM_ERR_UNSUPPORTED, the message
 *   starting "tvam_forward_dprojector: " / "tvam_adjoint_dprojector: " and naming the cause (a
 *   collimated projector, a traced 'cylindrical' / 'square' vial, a 'custom' or 'double_cylindrical'
 *   vial, dielectric occluders, occluders, albedo > 0, the ratio / delta sensors, a surface-aware film,
 *   a film slab).  A param outside TVAM_DPROJ_* or a null pointer: TVAM_ERR_INVALID.  All checks run
 *   before any device call; a refusal allocates nothing.
 */
#define TVAM_DPROJ_DISTANCE        0
#define TVAM_DPROJ_FOCUS_DISTANCE  1
#define TVAM_DPROJ_APERTURE_RADIUS 2
#define TVAM_DPROJ_PIXEL_SIZE      3
int tvam_forward_dprojector(tvam_plan* plan, int32_t param, const float* active_data,
                            const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                            float* tangent /* film, overwritten */, void* hip_stream);
int tvam_adjoint_dprojector(tvam_plan* plan, int32_t param, const float* active_data, const float* grad_dose,
                            const uint32_t* active_pixels, uint64_t n_active, uint32_t spp, uint32_t seed,
                            double* g /* device, overwritten */, void* hip_stream);

/* Update desc.active_base / desc.active_total of a plan (after the active set was
   compacted, e.g. by 'filter_radon', optimize.py:143-163); later calls seed and
   weight their rays with them. */
int tvam_plan_set_active(tvam_plan* plan, int64_t active_base, int64_t active_total);

/* Diagnostics (host-synchronous): number of (slice, tile) workgroups of the
   last forward that accumulated with float atomics instead of fixed point
   (needs TVAM_FLAG_FWD_STATS). */
int tvam_plan_stats(tvam_plan* plan, uint64_t* fallback_tiles);

/* Radon filter (integrators/radon.py:47-106, optimize.py:143-163, 'filter_radon'):
   for every DMD pixel of the plan's shard (dense crop order [angle][row][col],
   n = shard angles * crop_y * crop_x), the sum over `spp` samples of the ray
   weight times the absorption on the ray's segments inside both the medium
   and the target mesh (null BSDF); the optimiser keeps the pixels with a
   positive value.  target_tris: host array [n_target_tris][3][3] of
   world-space triangles.  radon: device, n floats, overwritten.  Synchronous. */
int tvam_radon(tvam_plan* plan, const float* target_tris, int32_t n_target_tris, uint32_t spp, uint32_t seed,
               int32_t max_depth, float* radon, void* stream);

/* Corner filter (integrators/filter_corner.py:17-66, optimize.py:166-185, 'filter_corner'): for
   every active entry, one ray through the centre of its pixel (regular sampling, spp 1, seed 0,
   no time sample, whatever the plan's own sampling is; 'telecentric' / 'lens' still take the
   aperture draw of sampler stream = the entry's position in the whole active set, as
   tvam_plan_set_active places this plan in it) is intersected with the scene's surfaces: the
   container's outer surface (index_matched: open tube r, cylindrical: open tube r_ext, both
   |z| <= height / 2 and hit from either side; square: the closed cuboid w_ext x w_ext x height)
   and the occluder triangles.  The target mesh, which the reference's scene also holds, lies
   inside the container and is left out.  keep[i] (device, f32, n_active entries, overwritten) =
   1 when the ray meets a surface at p and not sqrt((|p.x| - dist)^2 + (|p.y| - dist)^2) < radius,
   else 0.  hits (device, 16-byte aligned, [n_active][4] f32; may be NULL) = {p.x, p.y, p.z, t},
   {0, 0, 0, -1} on a miss.
     active_pixels : as in tvam_forward (u32 full-DMD indices), any pixel of the DMD; an entry
                     whose angle is outside the plan's angle shard is dropped (keep 0, t -1).
                     NULL: the plan's dense shard order [angle][crop row][crop col] (the row band
                     of a slab plan), n_active = shard angles * crop_y * crop_x.
   Asynchronous on hip_stream.  Every plan kind (projector, vial, occluders, scattering, slab or
   angle shard).  TVAM_ERR_INVALID: null plan / keep, radius < 0, non-finite dist, misaligned
   hits, n_active != the shard's size with active_pixels == NULL.  (Added to ABI v13: no struct or
   existing signature changed.) */
int tvam_corner(tvam_plan* plan, const uint32_t* active_pixels, uint64_t n_active,
                float dist, float radius, float* keep, float* hits, void* hip_stream);

/* Surface-aware discretisation (film_channels == 2; VolumetricSensor.compute_volume,
   sensor.py:47-110): volumes[z][y][x][2] (device, f32, overwritten) = the voxel volume
   inside (channel 0) / outside (1) the target mesh, estimated from sample_count points per
   voxel (independent sampler seeded (0, voxel)), each classified by the orientation of the
   first target hit along a uniform random direction.  Synchronous. */
int tvam_compute_volume(tvam_plan* plan, uint32_t sample_count, float* volumes, void* hip_stream);

/* Target discretisation (utils.py:83-128 discretize; the target transform of
   optimize.py:30-50 is applied by the caller): occ[z][y][x] (device, f32, overwritten)
   = 1 where the voxel centre bbox_min + (0.5 + i) h lies strictly inside the target
   mesh's bbox and the first hit of a ray from it along square_to_uniform_sphere(next_2d)
   (independent sampler seeded (0, voxels), lane = flat voxel index) faces away from the
   ray (dot(n, d) > 0), else 0.  Uses desc->film_res, bbox_min/max and target_tris
   (host, world space).  Runs on the current HIP device; synchronous. */
int tvam_discretize(const tvam_desc* desc, float* occ, void* hip_stream);

/* Diagnostics (host-synchronous): the fixed-point scale of the last forward of a plan
   served by the ray-driven planar forward (tvam_plan_path == 1): scale[0] = 2^e with
   |every voxel's scaled sum| < 2^30 guaranteed, scale[1] = 1 (exact int32 fixed point)
   or 0 (the bound was not finite: float LDS adds). */
int tvam_plan_fwd_scale(tvam_plan* plan, float* scale);

/* Diagnostics (host-synchronous): the chunking of the last brick-binned call of a plan with
   a scattering medium (the later segments of every path, tvam_scatter.hip).  stats[0] =
   chunks of paths, [1] = chunks served from the forward bin cache (weights rescaled to the
   new pattern, no replay / sort), [2] = chunks stored into the cache, [3] = brick entries
   marched, [4] = paths per chunk (all 0 when the plan's last call binned nothing), [5] = device
   bytes the forward bin cache holds, [6] = device bytes of the chunk scratch, [7] = slots whose
   bin-fill walk disagreed with the record writer's closed-form brick count, summed over the calls
   since the chunk scratch was allocated (0 by construction; host-synchronous read; a binned call
   that finds an earlier call's count nonzero fails with TVAM_ERR_HIP).  stats has 8 entries.
   (ABI v10) */
int tvam_plan_bin_stats(tvam_plan* plan, int64_t* stats);

/* Diagnostics (host-synchronous): the per-ray tile kernels' row walks for the plan's most
   recent ray records (jittered sampling).  stats[0] = rays the ray setup listed as strays
   (outside their row's main slice; -1 when the plan keeps no stray lists: regular sampling,
   rows whose interior jitters already change slice, or > 2^32 records), [1] = the stray-list
   capacity (beyond it every workgroup walks its slice's full row list), [2] = the (tile, slice)
   workgroups' stray walk summed over the launch (each walks its slice's whole stray list:
   strays x tiles), [3] = their main-row slot walk (rows x slots x spp over all workgroups),
   [4] = frozen-axis rays, [5] = spp of the records, [6] = tiles, [7] = (angle, column) slots
   over all tiles.  stats has 8 entries.  (ABI v11) */
int tvam_plan_tile_stats(tvam_plan* plan, int64_t* stats);

/* Measurement (host-synchronous): launch time of the plan's dominant forward kernel -- the
   forward brick march of a scattering medium, else the voxel-driven planar forward where it
   serves, else the per-ray tile forward -- from HIP events recorded on its stream around each
   launch.  Returns the launches recorded since the previous call and their summed time in ms (at
   most 1024 per measurement), then stops recording, or (enable != 0) starts a new measurement of
   the kernel kind of `plan`.  One timer per process, owned by the plan that enabled it (another
   plan's call fails while it runs; launches on other devices are not recorded); reading it
   (enable == 0) releases it, and so does destroying the owning plan.  (ABI v11) */
int tvam_plan_kernel_time(tvam_plan* plan, int32_t enable, double* total_ms, int64_t* launches);

/* Surface-aware plans: the per-channel voxel volumes the forward divides by and the
   adjoint multiplies the incoming gradient with (inv_vol = 1/volume, 0 where volume
   is 0: volume.py:41-42, :130).  Device pointer [z][y][x][2], caller-owned, kept by
   the plan until replaced; must be set before tvam_forward / tvam_adjoint. */
int tvam_plan_set_volumes(tvam_plan* plan, const float* volumes);

/* Which kernels serve this plan (bit mask; 0 = per-ray tile kernels):
   bit 0 = planar adjoint (regular sampling: one ray record per (angle,
   column), Z-slice-sharing adjoint); bit 1 = voxel-driven planar forward
   (straight rays only: not behind a refracting vial); bit 2 = 3-D projector
   rays (telecentric / lens: tvam_ray3d.hip; ABI v13). */
int tvam_plan_path(const tvam_plan* plan);

/* Diagnostics: the instantiation of the voxel-driven forward kernel that the plan launches (the
   launcher dispatches on the same record).  v[8] = slices per workgroup Z, candidate columns NC the
   kernel is instantiated for, the plan's candidate count nc (1 is served by NC = 2; behind a
   refracting vial the largest per-(tile, angle) count), staged window columns ncmax, angles per
   barrier AB, staged values (binned: float4s) per thread PF, flags (bit 0 BIN: staged from the
   slice-binned patterns, 1 DMA: by LDS-DMA, 2 MULTI: the direct staging sums several DMD rows per
   slice, 3 REFR: refracted chords, 4 SCONST: per-angle constants in scalar registers), angle parts
   per (tile, slice chunk).  TVAM_ERR_UNSUPPORTED when the voxel-driven forward does not serve the
   plan (tvam_plan_path bit 1 clear).  (Added to ABI v13: no struct or existing signature changed.) */
int tvam_plan_fwd_variant(const tvam_plan* plan, int32_t* v);

/*
 * Fused vector kernels of the linear L-BFGS step (lbfgs.py:146-275,
 * optimize.py:316-318).  All vectors are f32, n entries, 16-byte aligned.
 *
 * tvam_lbfgs_history: with p_old != NULL forms s_new = p - p_old and
 *   y_new = g - g_old (written to s_new / y_new) and, over the h retained
 *   pairs S[j], Y[j] (oldest first, 0 <= h <= 7) followed by the new pair,
 *   writes to dots (f64): s_j.g | y_j.g | s_new.y_j | s_j.y_new | y_new.y_j
 *   (h + 1 entries each) | g.g.  With p_old == NULL only s_j.g | y_j.g | g.g
 *   (h entries each).  With p_old == NULL and g_old != NULL (ABI v12): the new
 *   pair's s_new already holds p - p_old (tvam_axpy_clamp_dev's s_out) and is
 *   read, y_new formed; the same dots as the p_old path.  work: >=
 *   TVAM_LBFGS_WORK_DOUBLES f64 of scratch.
 * tvam_lbfgs_direction: d = cg g + sum_j (cs[j] S[j] + cy[j] Y[j]), h <= 8.
 * tvam_axpy_clamp: out = max(p + alpha d, lo) (out may alias p).
 * tvam_lbfgs_coef: the two-loop recursion (lbfgs.py:221-243) on the device, in
 *   Gram form, one lane: order[h] = the ring slots (0..7) of the pairs, oldest
 *   first, the new pair last when is_new; dots = tvam_lbfgs_history's output
 *   for those pairs (device, after any all-reduce); gram (device, 128 f64) keeps
 *   s_a.y_b / y_a.y_b by slot across steps (the new pair's entries are stored
 *   into it).  Writes coef (device, 17 f32: cg | cs[8] | cy[8]) and gdz (device
 *   f64: g.d).  first: the first step (gamma = 1).  No host synchronisation.
 * tvam_lbfgs_direction_dev: tvam_lbfgs_direction with coef read from device
 *   memory (tvam_lbfgs_coef's output).
 * tvam_lbfgs_history_rows: tvam_lbfgs_history over the entries seg_off +
 *   a * seg_stride + [0, seg_len) of every a < nseg only (a band of DMD rows):
 *   s_new / y_new of those entries and the band's dots (summed over the bands by
 *   the caller, in band order, before tvam_lbfgs_coef).
 * tvam_lbfgs_direction_rows: the same for the entries seg_off + a * seg_stride +
 *   [0, seg_len) of every a < nseg only (a band of DMD rows of every angle:
 *   seg_stride = rows * columns), so that the forward of one band's slices can
 *   start while the next band's direction is formed (all multiples of 4).
 * tvam_lbfgs_armijo: the first batch of backtracking Armijo probes (lbfgs.py:256-266)
 *   decided on the device, one lane: alpha[0] (device f32) = a_j = alpha0 / 2^j
 *   for the first j < nprobe with probes[j] <= loss + c1 a_j gdz[0] (device f64
 *   probes and g.d; loss = loss_dev[0] / loss_div, or loss_host when loss_dev is
 *   NULL), evaluated as the host loop evaluates it in f64; 0 when none passes.
 *   report (may be NULL; device-visible, e.g. pinned host memory the host polls):
 *   loss_dev[0] (or loss_host) | gdz[0] | probes[0..nprobe) | alpha | 1.0, f64, the
 *   final 1.0 written after the others are visible system-wide.
 * tvam_axpy_clamp_dev: tvam_axpy_clamp with alpha read from device memory
 *   (tvam_lbfgs_armijo's output), so the update follows the probes on the stream
 *   without a host round trip; s_out (may be NULL, no alias of p / d / out) =
 *   out - p, the next step's s_new.  (Both ABI v12.)
 * Pinned by tests/test_gpu_vec_kernels.py: the dots layout above, f64 accumulation of the exact f32
 *   products (error <= n 2^-53 sum|product|), and bit-identical dots for identical calls.
 */
#define TVAM_LBFGS_WORK_DOUBLES (2048 * 64)
int tvam_lbfgs_history(uint64_t n, const float* p, const float* p_old, const float* g, const float* g_old,
                       int32_t h, const float* const* S, const float* const* Y, float* s_new, float* y_new,
                       double* work, double* dots, void* hip_stream);
int tvam_lbfgs_history_rows(uint64_t nseg, uint64_t seg_len, uint64_t seg_stride, uint64_t seg_off, const float* p,
                            const float* p_old, const float* g, const float* g_old, int32_t h, const float* const* S,
                            const float* const* Y, float* s_new, float* y_new, double* work, double* dots,
                            void* hip_stream);
int tvam_lbfgs_direction(uint64_t n, const float* g, int32_t h, const float* const* S, const float* const* Y,
                         float cg, const float* cs, const float* cy, float* d, void* hip_stream);
int tvam_lbfgs_coef(int32_t h, int32_t is_new, int32_t first, const int32_t* order, const double* dots,
                    double* gram, float* coef, double* gdz, void* hip_stream);
int tvam_lbfgs_direction_dev(uint64_t n, const float* g, int32_t h, const float* const* S, const float* const* Y,
                             const float* coef, float* d, void* hip_stream);
int tvam_lbfgs_direction_rows(uint64_t nseg, uint64_t seg_len, uint64_t seg_stride, uint64_t seg_off,
                              const float* g, int32_t h, const float* const* S, const float* const* Y,
                              const float* coef, float* d, void* hip_stream);
int tvam_axpy_clamp(uint64_t n, const float* p, float alpha, const float* d, float lo, float* out,
                    void* hip_stream);
int tvam_axpy_clamp_dev(uint64_t n, const float* p, const float* alpha, const float* d, float lo, float* out,
                        float* s_out, void* hip_stream);
int tvam_lbfgs_armijo(int32_t nprobe, double alpha0, const double* probes, const double* loss_dev, double loss_host,
                      double loss_div, const double* gdz, double c1, float* alpha, double* report,
                      void* hip_stream);

/*
 * First-order optimiser updates (Mitsuba's mi.ad.SGD / mi.ad.Adam for one parameter and a scalar
 * learning rate; drtvam_amd/optimizers.py), fused with the loop's clamp (optimize.py:320).  All
 * vectors are f32, n entries, updated in place; any 4-byte alignment is accepted (vectors sharing
 * one offset from the 16-byte grid take the float4 path).  Hyper-parameters arrive as doubles and
 * are rounded inside: lr32 = fl32(lr), mu = fl32(momentum), b = fl32(beta), c = fl32(1 - beta)
 * with the subtraction in double, e = fl32(epsilon).  Per element every operation is one
 * once-rounded f32 operation in the written order (no fma); keep = mask && g == 0:
 * tvam_sgd_step: s == NULL (momentum must be 0): w = p - lr32 g.  Else s' = mu s + g;
 *   w = p - lr32 s'; keep: s' = s.  Then keep: w = p; p' = w < lo ? lo : w.
 * tvam_adam_step: m' = b1 m + c1 g; v' = b2 v + c2 (g g); keep: m' = m, v' = v;
 *   den = sqrt(v') + e; w = p - (lr_t m') / den; keep: w = p; p' = w < lo ? lo : w.
 *   lr_t = fl32(fl32(lr) fl32(sqrt(1 - beta_2^t) / (1 - beta_1^t))) is the caller's, for its step
 *   count t.
 * tvam_adam_moments / tvam_adam_apply: Adam with uniform = True in two passes.  The moments pass
 *   updates m and v as above and writes S[0] (device f64) = sum v', accumulated in f64 per thread,
 *   per block, then over the blocks in block order (deterministic); work: >=
 *   TVAM_LBFGS_WORK_DOUBLES f64 of scratch.  The caller may all-reduce S.  The apply pass reads
 *   S[0] and count[0] (device f64: the entries of all ranks) and takes den = fl32(sqrt(S / count))
 *   + e (quotient and root in f64) for every element; g is read only with mask (else may be
 *   NULL).  No host round trip between the two.
 * n == 0 returns 0 without a launch; a NULL required pointer returns TVAM_ERR_INVALID.
 * Pinned by tests/test_gpu_optimizers.py: p, s, m, v bit for bit against the f32 model of
 *   tests/optim_model.py, S within n 2^-53 sum|v'| and bit-identical for identical calls.
 */
int tvam_sgd_step(uint64_t n, float* p, const float* g, float* s, double lr, double momentum, int32_t mask,
                  float lo, void* hip_stream);
int tvam_adam_step(uint64_t n, float* p, const float* g, float* m, float* v, double lr_t, double beta_1,
                   double beta_2, double epsilon, int32_t mask, float lo, void* hip_stream);
int tvam_adam_moments(uint64_t n, const float* g, float* m, float* v, double beta_1, double beta_2, int32_t mask,
                      double* work, double* S, void* hip_stream);
int tvam_adam_apply(uint64_t n, float* p, const float* g, const float* m, const double* S, const double* count,
                    double lr_t, double epsilon, int32_t mask, float lo, void* hip_stream);

/* Global film z-slice of every crop row's rays under regular sampling
   (slice_of_row[crop_y]; -1 when the row's rays miss the grid or the vial),
   computed with the plan's own fp32 ray generation: the row <-> slice map
   that z-slab sharding of planar scenes partitions. */
int tvam_row_slices(const tvam_desc* desc, int32_t* slice_of_row);

/* The planar adjoint of film slices [z_begin, z_end) alone (tvam_adjoint of a dense set restricted
   to them), into DMD rows [row_begin, row_end) of every angle of grad_active (n_active = the dense
   crop count; those rows zeroed first, the others untouched).  The rows must be exactly the rows
   whose rays lie in those slices (tvam_row_slices); slices on tvam_plan_adj_chunk's chunks.  With
   tvam_forward_slices it lets a caller pipeline a slab's forward, loss and adjoint with the vector
   passes of the neighbouring slabs.  TVAM_ERR_UNSUPPORTED off the planar path. */
int tvam_adjoint_slices(tvam_plan* plan, const float* grad_dose, uint64_t n_active, int32_t z_begin, int32_t z_end,
                        int32_t row_begin, int32_t row_end, float* grad_active, void* hip_stream);
/* Slice granularity of tvam_adjoint_slices (0: not available). */
int tvam_plan_adj_chunk(const tvam_plan* plan);

/*
 * Diagnostics (ABI v13): the projector rays of a call, as tvam_forward / tvam_adjoint generate them
 * (get_ray projector.py:184-188, :220-234, :273-286; to_world motion.py:26-36; the medium segment
 * volume.py:191-216).  rays: device, [n_active * spp][16] f32, row active entry * spp + sample
 * (sampler-stream order) = o[3], d[3], hit (0 / 1), o2[3], maxt, d2[3], weight, 0: the ray, whether
 * it deposits, its medium segment (o2, d2, [0, maxt]) and its whole weight (inv_pdf / n_samples *
 * print_time * sigma_a / sigma_t; multiply by the pattern value and 1 / voxel volume for the dose).
 * active_pixels as in tvam_forward (NULL: the dense crop order).  All three projector kinds on
 * index-matched plans with a non-scattering medium, and on 'custom' and 'double_cylindrical' vial
 * plans, whose d2 is the refracted direction and whose weight carries the product of the
 * interfaces' transmission weights (double_cylindrical: the first of the two segments, see
 * tvam_plan_segments); TVAM_ERR_UNSUPPORTED otherwise.
 */
int tvam_plan_rays(tvam_plan* plan, const uint32_t* active_pixels, uint64_t n_active, uint32_t spp,
                   uint32_t seed, float* rays, void* hip_stream);

/* Exact number of DDA voxel visits of one pass (host-synchronous). */
int tvam_count_visits(tvam_plan* plan, uint32_t spp, uint32_t seed,
                      uint64_t* visits);

/*
 * ThresholdedLoss (loss.py:82-132) over a binary target, fused.
 *   x = dose + alpha * ddose (ddose may be NULL), target: f32 (>0 = object).
 *   out[0] += sum of the per-voxel loss (f64 accumulation, caller zeroes out);
 *   grad (may be NULL) = dL/dx per voxel (sum reduction; scale = 1/n for mean
 *   is applied by the caller through `scale`).
 */
int tvam_loss_threshold(const float* dose, const float* ddose, float alpha,
                        const float* target, uint64_t n, int32_t K,
                        float tl, float tu, float w_object, float w_void,
                        float w_limit, float scale, double* out, float* grad,
                        void* hip_stream);

/*
 * Armijo probes of LinearLBFGS's line search (lbfgs.py:255-268), fused: the
 * ThresholdedLoss of dose + alphas[j] * ddose for j < n_alpha (<= 8, alphas on
 * the host) in one pass; out[j] += the sum for alphas[j] (f64, caller zeroes
 * out[0..n_alpha)), scaled like tvam_loss_threshold.  Per element the same
 * arithmetic as tvam_loss_threshold with that alpha.
 */
int tvam_loss_threshold_probes(const float* dose, const float* ddose,
                               const float* alphas, int32_t n_alpha,
                               const float* target, uint64_t n, int32_t K,
                               float tl, float tu, float w_object, float w_void,
                               float w_limit, float scale, double* out,
                               void* hip_stream);

/*
 * The object test of both loss kernels (target > 0, loss.py:119) from a bit mask
 * of the target, 1/32 of its bytes (ABI v12):
 *   tvam_target_mask: mask[(n + 31) / 32] (device u32), bit j of word w =
 *   target[32 w + j] > 0 (0 past n).
 *   tvam_loss_threshold_mask / tvam_loss_threshold_probes_mask: tvam_loss_threshold /
 *   tvam_loss_threshold_probes with voxel i's object bit read at bit mask_bit0 + i
 *   of mask (a slab of the film: mask_bit0 = its first voxel's index).
 */
int tvam_target_mask(const float* target, uint64_t n, uint32_t* mask, void* hip_stream);
int tvam_loss_threshold_mask(const float* dose, const float* ddose, float alpha,
                             const uint32_t* mask, uint64_t mask_bit0, uint64_t n, int32_t K,
                             float tl, float tu, float w_object, float w_void,
                             float w_limit, float scale, double* out, float* grad,
                             void* hip_stream);
int tvam_loss_threshold_probes_mask(const float* dose, const float* ddose,
                                    const float* alphas, int32_t n_alpha,
                                    const uint32_t* mask, uint64_t mask_bit0, uint64_t n,
                                    int32_t K, float tl, float tu, float w_object,
                                    float w_void, float w_limit, float scale,
                                    double* out, void* hip_stream);

/*
 * L2Loss over a one-channel target, and ThresholdedLoss / L2Loss over a surface-aware (two-channel)
 * film, fused (loss.py:28-59, :62-79, :82-132).  (Added to ABI v13: no struct or existing signature
 * changed.)  x = dose + alpha * ddose as one fmaf (ddose may be NULL in the value entries);
 * out[0] += scale * sum of the per-voxel elements (f64 accumulation, the caller zeroes out); grad (may
 * be NULL) = dL/dx per float, times scale (scale = 1 / voxels of the whole film for 'mean', the
 * caller's to supply: the reduction counts voxels, not floats).  Any 4-byte alignment; float4
 * accesses when every pointer is 16-byte aligned.  Per element, fp32 operations in this order,
 * none contracted:
 *
 *   tvam_loss_square: n floats each.  d = x - target; element d * d; grad = (2 * d) * scale.  target
 *   is the greyscale f32 target itself (no bit mask).
 *
 *   tvam_loss_surface: dose, ddose, target, grad hold 2 * n_vox floats, interleaved per voxel: x0, x1
 *   (dose inside / outside the object) and t0 = V_in, t1 = V_out.  s = t0 + t1, w_in = t0 / s, w_out =
 *   t1 / s (IEEE divisions; a voxel with s = 0 is outside the contract, 0 / 0 as in the reference).
 *   element = w_in * e_in + w_out * e_out; grad[2 i] = (w_in * g_in) * scale, grad[2 i + 1] = (w_out *
 *   g_out) * scale, with
 *     kind TVAM_LOSS_KIND_THRESHOLD: e_in = w_object relu(tu - x0)^K + w_limit relu(x0 - 1)^K, e_out =
 *       w_void relu(x1 - tl)^K and their derivatives as in tvam_loss_threshold (0 at a kink), integer
 *       K in [1, 16];
 *     kind TVAM_LOSS_KIND_L2: e_in = (x0 - 1)^2, e_out = x1^2, g_in = 2 (x0 - 1), g_out = 2 x1 (K, tl,
 *       tu and the weights are ignored).
 *
 *   tvam_loss_square_probes / tvam_loss_surface_probes: the values at dose + alphas[j] * ddose for j <
 *   n_alpha (<= 8, alphas on the host) in one pass, out[j] += the scaled sum (the caller zeroes
 *   out[0..n_alpha)).  Per element the same arithmetic as the value entry with that alpha.
 *
 * TVAM_ERR_INVALID (the message names the entry and the cause): null dose, target or out; for the
 * probes null ddose or alphas, n_alpha outside [1, 8]; an unknown kind; K outside [1, 16] with the
 * threshold kind.  n == 0 launches nothing and leaves out untouched.
 */
#define TVAM_LOSS_KIND_THRESHOLD 0
#define TVAM_LOSS_KIND_L2 1
int tvam_loss_square(const float* dose, const float* ddose, float alpha, const float* target,
                     uint64_t n, float scale, double* out, float* grad, void* hip_stream);
int tvam_loss_square_probes(const float* dose, const float* ddose, const float* alphas,
                            int32_t n_alpha, const float* target, uint64_t n, float scale,
                            double* out, void* hip_stream);
int tvam_loss_surface(int32_t kind, const float* dose, const float* ddose, float alpha,
                      const float* target, uint64_t n_vox, int32_t K, float tl, float tu,
                      float w_object, float w_void, float w_limit, float scale, double* out,
                      float* grad, void* hip_stream);
int tvam_loss_surface_probes(int32_t kind, const float* dose, const float* ddose,
                             const float* alphas, int32_t n_alpha, const float* target,
                             uint64_t n_vox, int32_t K, float tl, float tu, float w_object,
                             float w_void, float w_limit, float scale, double* out,
                             void* hip_stream);

/*
 * The print report's primitive (drtvam_amd/utils.py: iou_sweep, save_histogram; the reference's
 * save_histogram, utils.py:8-11, :48-81).  (Added to ABI v13: no struct or existing signature changed.)
 *
 * Class-split histogram of x over a sorted edge table.
 *   class c(i) = target[i] > 0 ? 1 : 0        (object / empty, utils.py:9,50)
 *   slot  j(i) = side == 0 ? #{k : edges[k] <  x[i]}  (so x > edges[k]  <=>  k < j)
 *                          : #{k : edges[k] <= x[i]}  (half-open bins [e_k, e_k+1))
 *   counts[c][j] for j in 0..n_edges; counts[c][n_edges+1] = number of NaN x (NaN takes no slot).
 *   x, target: device, n floats, any 4-byte alignment.  edges: HOST, n_edges floats.
 *   counts: device, uint64 [2][n_edges + 2], zeroed by the call.  Synchronises the stream.
 * The slot comes from fp32 compares alone, so it is exact: -0 equals 0, +-inf land in slot 0 or
 * n_edges, denormals compare as themselves.  Integer counts: the result does not depend on the order
 * of the adds.  TVAM_ERR_INVALID (the message names the cause) for a null pointer, n_edges outside
 * [1, 2048], a non-finite edge, edges that are not strictly increasing, or side not in {0, 1}.
 * n == 0 (x and target may then be NULL) zeroes counts and launches nothing.
 */
int tvam_class_hist(const float* x, const float* target, uint64_t n, const float* edges,
                    int32_t n_edges, int32_t side, uint64_t* counts, void* hip_stream);

/* Thread-local message describing the last error ("" if none). */
const char* tvam_last_error(void);

/* ABI version of the loaded library. */
int tvam_abi_version(void);

/* Bytes of device memory the library owns in this process, over all plans and devices: the plans'
   tables, ray records, scratch and caches, and the temporaries of a running call.  0 before the
   first plan and again after the last tvam_plan_destroy.  (Added to ABI v13: no struct or existing
   signature changed.) */
int64_t tvam_device_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* TVAM_H_ */
