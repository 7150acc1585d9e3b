/*
 * mcpt.h -- C ABI of the MI355X-native path-tracing hot path (libmcpt_hip.so).
 *
 * The reference (a single C++ executable) has no plugin/FFI interface; its only seam around the hot
 * path is the C++ call  Renderer::Render(const Scene&)  (src/Renderer.hpp:16, called once at
 * src/main.cpp:333) configured through Renderer::setSpp (Renderer.hpp:18) and the Scene setters
 * (Scene.hpp:104-119).  The entry points below are exactly what a binding for that seam needs; each
 * one names the reference interface it replaces.  Plain pointers and sizes only: no C++ or torch types.
 *
 * All functions return 0 on success or an mcpt_status code; mcpt_last_error() returns a thread-local
 * description of the last failure.  A scene handle may be used by one host thread at a time.
 * The library never falls back to a CPU path: without a usable HIP device every call fails with
 * MCPT_ERR_HIP.
 */
#ifndef MCPT_H
#define MCPT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MCPT_OK = 0,
    MCPT_ERR_ARG = 1,      /* bad argument / inconsistent description */
    MCPT_ERR_HIP = 2,      /* HIP runtime error (no device, launch failure, ...) */
    MCPT_ERR_OOM = 3,      /* host or device allocation failed */
    MCPT_ERR_LIMIT = 4,    /* a compiled-in limit was exceeded (BVH depth, light-tree depth) */
    MCPT_ERR_OVERFLOW = 5  /* a path outran the clamp stack (params.max_depth); frame is still returned */
} mcpt_status;

/* MaterialType, src/Material.hpp:13-18 */
enum { MCPT_SMOOTH_CONDUCTOR = 0, MCPT_ROUGH_CONDUCTOR = 1, MCPT_SMOOTH_DIELECTRIC = 2, MCPT_ROUGH_DIELECTRIC = 3 };
enum { MCPT_OBJ_MESH = 0, MCPT_OBJ_SPHERE = 1 };

/* One Triangle of a MeshTriangle (src/Triangle.hpp:41-56, 99-124): world-space vertices, texture coords. */
typedef struct {
    float v0[3], v1[3], v2[3];
    float t0[2], t1[2], t2[2];
} mcpt_triangle; /* 60 bytes */

/* src/Material.hpp:157-167 (+ ctor defaults :245-257): the fields the hot path reads. */
typedef struct {
    int32_t type;
    int32_t textured; /* checkerboard reflectance, Material.hpp:134-151 */
    float roughness, iorA, iorB;
    float base_reflectance[3];
    float emission[3];
} mcpt_material; /* 44 bytes */

/* One Scene::Add()-ed Object (src/Scene.hpp:104-109): a MeshTriangle or a Sphere (src/Sphere.hpp:10-21). */
typedef struct {
    int32_t kind;      /* MCPT_OBJ_MESH | MCPT_OBJ_SPHERE */
    int32_t material;  /* index into materials */
    int32_t first_tri; /* mesh: first triangle in `triangles`, file order */
    int32_t n_tri;     /* mesh: triangle count */
    float center[3];   /* sphere */
    float radius;      /* sphere */
} mcpt_object; /* 32 bytes */

/* Everything Scene holds once main() has assembled it (src/Scene.hpp:32-38,147-149). Borrowed pointers:
 * the library copies what it needs into HBM; the caller keeps ownership. */
typedef struct {
    int32_t n_objects;
    int32_t n_triangles;
    int32_t n_materials;
    int32_t env_w, env_h;          /* 0,0 => constant background colour (Scene.hpp:33,61-63) */
    float background[3];
    const mcpt_object *objects;    /* in Scene::Add order */
    const mcpt_triangle *triangles;
    const mcpt_material *materials;
    const float *env_pixels;       /* env_w*env_h*3 floats in [0,1], row-major (Scene.hpp:48-56) */
} mcpt_scene_desc;

/* src/Camera.hpp:6-26 after lookAt(). */
typedef struct {
    int32_t width, height;
    float fov;            /* degrees */
    float position[3];
    float orientation[9]; /* row-major 3x3, columns = left, up, forward (Camera.hpp:21-23) */
    int32_t use_dof;
    float focal_distance, aperture_radius;
} mcpt_camera; /* 72 bytes */

/* Renderer::spp (Renderer.hpp:18,22) + the private Scene knobs (Scene.hpp:25-28,110-119) + launch shape. */
typedef struct {
    int32_t spp;           /* samples per pixel rendered by this call */
    int32_t spp_total;     /* divisor of `framebuffer += rgb/spp` (Renderer.cpp:80); 0 => spp */
    int32_t sample_offset; /* index of this call's first sample (progressive accumulation); RNG key uses offset+k */
    float rr_rate;         /* caller applies min(rr, 0.99f) as Scene::setRrRate does */
    int32_t n_dir_sample;  /* Scene::n_dir_sample (the reference always runs 4) */
    int32_t enable_shadow;
    uint32_t seed;
    int32_t accumulate;    /* 0: framebuffer is overwritten for owned pixels; 1: added to */
    /* pixel-tile partition (multi-GPU): pixel (i,j) is owned iff ((j/tile)*ceil(W/tile) + i/tile) % nranks == rank */
    int32_t tile_size, rank, nranks;
    /* launch shape; 0 => library default */
    int32_t spp_per_pass;  /* samples per pixel in flight per pass (sizes the per-pass result buffer); 0: chosen by the library so that a pass carries many pools of samples */
    int32_t pool_paths;    /* wavefront pool capacity in channel-paths */
    int32_t max_depth;     /* clamp-stack levels per path; 0 => derived from rr_rate (P[deeper] < 1e-12) */
} mcpt_params;

typedef struct {
    uint64_t samples;       /* camera samples */
    uint64_t paths;         /* channel paths = 3 * samples */
    uint64_t vertices;      /* Scene::castRay invocations the reference would execute (Scene.cpp:85) */
    uint64_t shaded;        /* vertices that reached Material::sample (Scene.cpp:109) */
    uint64_t closest_rays;  /* closest-hit rays actually traced (primary once per sample + continuations) */
    uint64_t shadow_rays;   /* shadow rays actually traced (light samples with a non-zero contribution) */
    uint64_t ref_scene_rays;/* Scene::intersect calls the reference would make for the same work */
    uint64_t iterations;    /* wavefront iterations */
    uint64_t overflow_paths;/* paths cut by max_depth */
    double ms_total;        /* wall time of the call, host clock */
    double ms_trace_closest, ms_trace_shadow, ms_shade, ms_generate, ms_resolve; /* HIP-event sums per kernel class */
    uint64_t n_trace_closest, n_trace_shadow, n_shade, n_generate, n_resolve;    /* launches per kernel class */
    double ms_direct;   /* k_direct (direct-lighting kernel) */
    uint64_t n_direct;
    uint64_t direct_vertices; /* shaded vertices whose light samples were evaluated (the rest provably contribute 0) */
} mcpt_stats;

typedef struct mcpt_scene mcpt_scene;

/* Replaces Scene::Add + Scene::buildBVH (Scene.hpp:104-109, Scene.cpp:14-17) and MeshTriangle's per-mesh
 * BVHAccel (Triangle.hpp:128-134, BVH.cpp:27-93): builds the flattened BVH and uploads the scene to HBM
 * of the current (or `device`) GPU. */
int mcpt_scene_create(const mcpt_scene_desc *desc, int device, mcpt_scene **out);
void mcpt_scene_destroy(mcpt_scene *scene);

/* The same with an explicit choice of the tree builder (mcpt_scene_create: options == NULL).  Closest-hit results do not depend on
 * the tree (equal distances go to the larger primitive id); only rays that graze a box face within float rounding can differ.
 *   MCPT_BUILD_SAH        host, binned SAH over all primitives (default)
 *   MCPT_BUILD_REFERENCE  host, the reference's two-level median-split topology (BVH.cpp:27-93), flattened
 *   MCPT_BUILD_GPU_LBVH   on the device: Morton-code linear BVH (radix sort + Karras hierarchy + bottom-up refit); milliseconds
 *   MCPT_BUILD_GPU_PLOC   on the device: parallel locally-ordered clustering over the same Morton order (merges chosen by surface area:
 *                         a tree of near-SAH quality in a few milliseconds; search radius MCPT_PLOC_RADIUS, default 16)
 *                         instead of seconds for large scenes, at a lower tree quality
 * Fields left at MCPT_BUILD_DEFAULT / -1 take the environment overrides MCPT_BVH = sah | reference | lbvh | ploc and
 * MCPT_QUANT_NODES = 0 | 1, then the defaults. */
enum { MCPT_BUILD_DEFAULT = 0, MCPT_BUILD_SAH = 1, MCPT_BUILD_REFERENCE = 2, MCPT_BUILD_GPU_LBVH = 3, MCPT_BUILD_GPU_PLOC = 4 };
typedef struct {
    int32_t builder;  /* MCPT_BUILD_* */
    int32_t quantise; /* -1 automatic, 0 float nodes (64 B), 1 quantised nodes (32 B) */
    /* Node instancing (host SAH builder only).  Meshes that are translated copies of one another -- the 14 soldiers of main.cpp:248-271
     * are one OBJ file at 14 positions -- share ONE subtree of traversal nodes, entered with the ray origin shifted; every primitive test
     * still uses the object's own world-space triangle as the reference stores it (Triangle.hpp:99-124), so hits are unchanged.  It is
     * a memory feature (the 296 k-triangle scene: 56.9 -> 31.3 MB in HBM), measured slower than the plain tree on MI355X, so the default
     * (MCPT_INSTANCING_AUTO) leaves it off. */
    int32_t instancing; /* MCPT_INSTANCING_AUTO (0) | MCPT_INSTANCING_OFF (1) | MCPT_INSTANCING_ON (2); env override MCPT_INSTANCING = 0 | 1 */
    int32_t reserved[5];
} mcpt_build_options;
enum { MCPT_INSTANCING_AUTO = 0, MCPT_INSTANCING_OFF = 1, MCPT_INSTANCING_ON = 2 };
int mcpt_scene_create_ex(const mcpt_scene_desc *desc, int device, const mcpt_build_options *options, mcpt_scene **out);

/* ---- Moving objects in a live scene.  The reference has no counterpart: its Scene is assembled once.
 *
 * mcpt_scene_update gives the listed objects a transform and rebuilds the traversal tree with the scene's own builder (never a refit).
 *   Point transform, in float, no contraction (m row-major 3x4):
 *       p'[r] = (m[4r]*p.x + (m[4r+1]*p.y + m[4r+2]*p.z)) + m[4r+3]            (the 3-term dot order, then the translation)
 *   Meshes   every stored vertex of the object's triangles is transformed, the texture coordinates are kept.  Any finite affine map is
 *            allowed: edges, normals and areas are derived from the moved vertices exactly as at creation (a reflection flips the
 *            normals, as it would in a fresh scene).
 *   Spheres  the centre is transformed, the radius is kept: the linear part acts on the centre only, spheres are not scaled.
 *   Transforms are ABSOLUTE: they apply to the geometry the scene was created with and never accumulate.  An object listed in a call
 *   gets that transform; an object not listed keeps the one it had; an object that never got one keeps its stored vertices bit for bit
 *   (no identity is applied: -0 + 0 would change a sign bit).
 * THE CONTRACT: after the call every entry point that takes the scene gives what it gives on
 *       mcpt_scene_create_ex(desc', device, the same options)
 * where desc' is the creation description with the current transforms applied by the rule above (what mcpt_transform_triangles
 * computes): mcpt_render*, mcpt_intersect, mcpt_cast_rays, mcpt_render_aovs*, mcpt_render_denoised, mcpt_scene_dump_bvh,
 * mcpt_debug_scene, and mcpt_scene_get_info in n_nodes, bvh_height, quantised, lds_resident, n_lights and n_prims.  With the host
 * builders (MCPT_BUILD_SAH, MCPT_BUILD_REFERENCE) bit for bit, the tree dump included; with the device builders as far as two builds
 * on the device agree: primitive ids equal ray for ray, a frame within a few values of a box-grazing ray.
 * The handle, its streams and events and the wavefront workspaces survive; no workspace is reallocated because of an update.
 *   info->path 0  host: desc' is flattened and its tree built as at creation, the geometry-derived arrays are copied to the device again
 *                 (every host-built scene; a device-built scene when a listed object emits light: the light tables are host-built)
 *   info->path 1  device: a kernel moves the listed triangles and sphere centres in HBM from the resident creation-time triangles and
 *                 the device builder runs again; only the matrices cross the bus
 * MCPT_ERR_ARG, before any device call: n < 0; n > 0 with moves == NULL; a matrix entry that is not finite; an object listed twice in
 * one call; scene == NULL; an object index out of range; a scene built with node instancing on (instanced subtrees are shared between
 * objects).  n == 0 is a valid no-op.  A failed rebuild (MCPT_ERR_LIMIT: the new tree is deeper than the traversal stack;
 * MCPT_ERR_OOM) leaves the scene exactly as it was before the call: the new arrays are built aside and swapped in on success. */
typedef struct { int32_t object; float m[12]; } mcpt_object_transform; /* 52 bytes; m row-major 3x4 */
typedef struct {
    int32_t path;         /* 0: host rebuild + re-upload, 1: device transform + device rebuild, 2: in place (mcpt_scene_set_*) */
    int32_t n_moved_tris; /* triangles of the listed meshes */
    double transform_ms;  /* path 0: forming desc' on the host; path 1: the segment table's copy and the transform kernel */
    double build_ms;      /* flattening + tree build (host and device parts) */
    double upload_ms;     /* path 0: host -> HBM copies; path 1: the device-to-device copies into the new arrays */
    double total_ms;      /* wall time of the call */
    int32_t reserved[4];
} mcpt_update_info; /* 56 bytes */
int mcpt_scene_update(mcpt_scene *scene, int32_t n, const mcpt_object_transform *moves, mcpt_update_info *info /* nullable */);
/* Host only, no GPU needed: out[i] = in[i] with its three vertices moved by the point transform above (uv copied); in == out allowed.
 * MCPT_ERR_ARG for m == NULL, a matrix entry that is not finite, n < 0, or n > 0 with a null array. */
int mcpt_transform_triangles(const float m[12], int64_t n, const mcpt_triangle *in, mcpt_triangle *out);

/* ---- Deforming meshes in a live scene: per-vertex updates from host or device memory.
 *
 * mcpt_scene_deform gives the listed meshes new vertex positions and rebuilds the traversal tree with the scene's own builder, exactly
 * as mcpt_scene_update does (one rebuild serves both).
 *   A deformation replaces the object's BASE geometry, the thing absolute transforms apply to.  The object's current transform, if it
 *   ever got one, keeps applying to the new base by the point rule above; a later mcpt_scene_update applies its matrix to the latest
 *   base.  An object that never got a transform stores the given floats bit for bit (the sign of a zero included).
 *   positions holds n_tri * 9 floats: v0, v1, v2 of each of the object's triangles, in the object's triangle order.  The triangle count,
 *   the triangle order, the texture coordinates and the material are unchanged.  Degenerate (zero-area) triangles are allowed, as at
 *   creation.
 *   on_device 0: positions is a host pointer.  on_device 1: a pointer into the memory of the scene's device (a PyTorch tensor, say), read
 *   in place by the kernel; the positions must be complete before the call (the caller synchronises its producer stream).  The call is
 *   blocking and works on the null stream, like mcpt_scene_update.
 * THE CONTRACT: after the call every entry point listed at mcpt_scene_update gives what it gives on
 *       mcpt_scene_create_ex(desc'', device, the same options)
 * where desc'' is the creation description with each deformed object's positions replaced by the latest ones given (what
 * mcpt_deform_triangles computes), then the current transforms applied (mcpt_transform_triangles).  With the host builders bit for bit,
 * the tree dump included; with the device builders by the rule stated there: primitive ids equal ray for ray, a frame within a few
 * values of a box-grazing ray.  Primitive ids are stable, so a snapshot taken before the call pairs every hit with the triangle's
 * previous vertices: mcpt_render_motion gives the motion of a triangle whose three vertices moved independently.
 *   info->path 1  device: the scene was built by MCPT_BUILD_GPU_LBVH or MCPT_BUILD_GPU_PLOC and no listed object emits light.  Host
 *                 positions cross the bus once, 36 bytes per triangle, into a staging buffer the scene owns; device positions are read
 *                 where they are.  One kernel forms the new base, applies the transforms and writes the records; the device builder
 *                 runs again.  The scene's host copy of the base follows at once: positions given by device pointer are copied back
 *                 (36 bytes per triangle) after the rebuild has succeeded, so that a later call on path 0 starts from the latest base.
 *   info->path 0  host: otherwise, exactly as for mcpt_scene_update.  Positions given by device pointer are downloaded first.
 *   info->n_moved_tris is the number of triangles of the listed meshes; the timing fields keep their meaning (on path 1 transform_ms
 *   covers the staging copy, the segment table and the kernel).
 * MCPT_ERR_ARG, before any device call: n < 0; n > 0 with items == NULL; a null positions; on_device not 0 or 1; an object listed twice in
 * one call; scene == NULL; an object index out of range; a sphere object; a scene built with node instancing on; a host position that
 * is not finite.  A position given by device pointer can only be checked once it is read: on path 1 the kernel raises one flag word
 * that the host reads before anything is swapped, on path 0 the downloaded copy is checked; either way the call returns MCPT_ERR_ARG.
 * n == 0 is a valid no-op.  Any failed call (MCPT_ERR_ARG, MCPT_ERR_LIMIT, MCPT_ERR_OOM) leaves the scene exactly as it was: the base
 * geometry on the host and on the device, the transforms, the live arrays and the snapshot.  The new base is built aside and committed
 * with the new tree. */
typedef struct {
    int32_t object;          /* a MESH object of the scene */
    int32_t on_device;       /* 0: positions is a host pointer; 1: a pointer into the scene's device */
    const float *positions;  /* n_tri * 9 floats: v0, v1, v2 of each triangle, in the object's triangle order */
} mcpt_object_vertices;      /* 16 bytes */
int mcpt_scene_deform(mcpt_scene *scene, int32_t n, const mcpt_object_vertices *items, mcpt_update_info *info /* nullable */);
/* Host only, no GPU needed: out[i] = in[i] with its nine position floats replaced by positions[9i .. 9i+9) (uv copied); in == out allowed.
 * MCPT_ERR_ARG for n < 0, or n > 0 with a null array. */
int mcpt_deform_triangles(int64_t n, const float *positions, const mcpt_triangle *in, mcpt_triangle *out);

/* ---- Relighting a live scene: materials, emitters and the sky edited in place.
 *
 * mcpt_scene_set_materials replaces the listed entries of the material table (materials[index] = material) and gives the listed objects
 * another entry of it (objects[object].material = material).  n_materials is fixed for the life of the scene: entries change, none is
 * added.  Both lists may be given in one call; they are applied together.
 * THE CONTRACT: after the call every entry point listed at mcpt_scene_update gives what it gives on
 *       mcpt_scene_create_ex(desc', device, the same options)
 * where desc' is the scene's current description (latest bases, current transforms) with the listed entries replaced and the listed
 * objects reassigned.  With the host builders bit for bit, the tree dump included; with the device builders by the rule stated there.
 * The scene's host copy of the description follows every successful call at once, so a later mcpt_scene_update / mcpt_scene_deform on
 * path 0 flattens the edited scene.  The snapshot of mcpt_scene_snapshot is not touched (it holds positions only).
 *   info->path 2  in place: every object emits light after the call if and only if it did before (Material::hasEmission of its
 *                 material).  Colour, roughness, ior, type, `textured`, the emission VALUES of a light that stays a light, reassignments
 *                 between non-emitting materials or between emitting ones.  The changed MaterialRecs are formed by the creation code and
 *                 copied into the table; one kernel rewrites the material words of the affected primitives (an object that was listed, or
 *                 a mesh whose material changed its `textured` flag); LightRec::mat of a reassigned emitter is patched.  The tree, the
 *                 node arrays and the host flatten are not touched: build_ms is 0.
 *   info->path 0  host: some object starts or stops emitting, so the light tables, the emitters' bounding sphere, n_lights and possibly
 *                 the LDS-resident decision change.  desc' is flattened and uploaded as on path 0 of mcpt_scene_update, for every builder,
 *                 together with the material table.
 *   info->n_moved_tris is the number of triangle records whose material words change; the timing fields keep their meaning
 *   (transform_ms: the table copy, the segment table and the kernel on path 2).
 * MCPT_ERR_ARG, before any device call: scene == NULL; a negative count, or a positive count with a null list; a material index or an
 * object index out of range; a material type outside 0..3; a material value that is not finite; the same material index, or the same
 * object, listed twice in one call; a scene built with node instancing on.  Both counts zero is a valid no-op.  A refused call, and a
 * call that fails on path 0, leaves the scene as it was: path 0 builds aside and swaps, path 2 does all its checking first, so only a HIP error can fail it afterwards.
 * After such an error (MCPT_ERR_HIP from a copy or the launch on path 2) the device tables may hold part of the edit while the host copy
 * of the description holds none of it, so a later host-path rebuild would drop that part: repeat the call, or destroy the scene.
 * Blocking, on the null stream, like mcpt_scene_update.  History kept by the caller (mcpt_temporal_*, mcpt_sequence_*) does not know
 * that the scene was relit: the colour clamp of mcpt_history_opts is the remedy for stale radiance, or mcpt_sequence_reset. */
typedef struct { int32_t index; mcpt_material material; } mcpt_material_edit;   /* 48 bytes: materials[index] = material */
typedef struct { int32_t object; int32_t material; } mcpt_object_material;      /* 8 bytes: objects[object].material = material */
int mcpt_scene_set_materials(mcpt_scene *scene, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign,
                             const mcpt_object_material *assign, mcpt_update_info *info /* nullable */);
/* mcpt_scene_set_environment replaces the background colour and the environment map (env_pixels: env_w * env_h * 3 floats as in
 * mcpt_scene_desc, or NULL with env_w == env_h == 0 for the constant colour).  Map <-> colour and a change of map size are allowed.  Always
 * in place (info->path 2, n_moved_tris 0): the new map is uploaded aside and swapped in on success; the sky cull, which only runs for a
 * constant background, reads the scene per call and switches by itself.  The same contract as above, with desc' the current description
 * with its background and environment replaced.  MCPT_ERR_ARG, before any device call: scene == NULL; background == NULL; env_w / env_h
 * not both zero with a null map, or not both positive with one; a background or map value that is not finite. */
int mcpt_scene_set_environment(mcpt_scene *scene, const float background[3], int32_t env_w, int32_t env_h, const float *env_pixels,
                               mcpt_update_info *info /* nullable */);

/* ---- Hiding and showing objects in a live scene: per-object visibility.
 *
 * mcpt_scene_set_visibility takes the primitives of hidden objects out of the traversal tree and, for emitters, out of the light tables.
 *   Visibility is ABSOLUTE and per object: an object listed in a call gets that state, an object not listed keeps the one it had, every
 *   object is visible after creation.  A hidden object keeps its records, its base geometry, its transform and its material where they
 *   are: mcpt_scene_update, mcpt_scene_deform and mcpt_scene_set_materials act on it as on any object (their path rules look at the
 *   listed objects as before, visible or not), it stays hidden until it is shown, and it then appears where those calls left it.
 *   Primitive ids never change: a triangle index, or n_triangles + object for a sphere.
 * THE CONTRACT: after the call every entry point listed at mcpt_scene_update gives what it gives on
 *       mcpt_scene_create_ex(compact(desc'), device, the same options)
 * where desc' is the scene's current description (latest bases, current transforms, current materials) and compact() is
 * mcpt_compact_scene with the scene's mask.  Primitive ids are translated through its prim_map: mcpt_intersect's out_prim, the leaves of
 * mcpt_scene_dump_bvh, the candidate ids of mcpt_debug_classify, the triangle ids of the light tables.  Everything else equals the fresh
 * scene bit for bit with the host builders (frames, mcpt_stats work counters, AOVs, motion, cast rays, light samples, node boxes and
 * quantised boxes), and by the rule of mcpt_scene_update with the device builders.
 *   mcpt_scene_get_info: n_nodes, bvh_height, quantised and n_lights are those of the fresh scene; n_prims stays the number of STORED
 *   records.  lds_resident is decided as at creation from the stored record counts and the new tree, since the stored arrays are what the
 *   LDS kernels copy: it can be 0 where the fresh compacted scene's is 1, never the other way round.
 *   info->path 1  device: the scene was built by MCPT_BUILD_GPU_LBVH or MCPT_BUILD_GPU_PLOC and no object whose state changes emits
 *                 light.  Only the tree is rebuilt, from the live triangles and sphere records: no record array is copied or written, and
 *                 only a table of the visible triangle ranges and the list of visible spheres cross the bus (transform_ms; build_ms is
 *                 the builder).
 *   info->path 0  host: every host-built scene, and any scene when an emitter is hidden or shown (the light tables, the emitters'
 *                 bounding sphere and n_lights change).  As path 0 of mcpt_scene_update; the creation code gets the mask and only
 *                 shortens the primitive lists it hands to the tree builders and the light table.
 *   info->n_moved_tris is the number of triangles of the meshes whose state changed.  A call after which no object's state differs
 *   (n == 0 included) rebuilds nothing and returns MCPT_OK with build_ms == 0.
 * MCPT_ERR_ARG, before any device call: scene == NULL; n < 0; n > 0 with items == NULL; an object index out of range; an object listed
 * twice in one call; visible not 0 or 1; a scene built with node instancing on; a result with no visible object (a scene cannot be
 * empty); on a device-built scene a result with fewer than two visible primitives (the device builders need two).  A refused call, and a
 * call whose rebuild fails (MCPT_ERR_LIMIT, MCPT_ERR_OOM), leaves the scene exactly as it was, mask included: the new tree is built aside
 * and swapped in on success.  Blocking, on the null stream, like mcpt_scene_update.
 * Temporal reuse: ids are stable, so the snapshot of mcpt_scene_snapshot keeps holding every record, hidden ones included, and keeps
 * pairing hits with previous positions.  An object shown again reports motion against where its records were at the snapshot, with
 * `valid` as for any object; the stale history behind it is rejected by the blend's depth validation and the colour clamp
 * (mcpt_history_opts), or by mcpt_sequence_reset. */
typedef struct { int32_t object; int32_t visible; } mcpt_object_visibility; /* 8 bytes; visible 0 | 1 */
int mcpt_scene_set_visibility(mcpt_scene *scene, int32_t n, const mcpt_object_visibility *items, mcpt_update_info *info /* nullable */);
/* The mask (visible: n_objects bytes, nullable; n_objects must then be the scene's object count) and the number of primitives in the
 * tree (nullable). */
int mcpt_scene_get_visibility(const mcpt_scene *scene, int32_t n_objects, uint8_t *visible /* nullable */, int32_t *n_visible_prims /* nullable */);
/* Host only, no GPU needed: the description without its hidden objects, which defines what a scene with that mask is compared with.
 * The visible objects are kept in their order and the triangles of the visible meshes in array order, with first_tri rewritten;
 * materials and the environment are the caller's own (not copied).  objects_out: room for n_objects, triangles_out: room for
 * n_triangles; both may be NULL to get the counts and the map only.  prim_map (nullable, n_triangles + n_objects entries): prim_map[p] is
 * the id live primitive p has in the compacted description, or -1 if it is hidden (entries n_triangles + o of mesh objects are -1 too).
 * The map is strictly increasing over the visible ids, so "the larger id wins a tie" means the same on both sides.
 * MCPT_ERR_ARG for a null desc or visible, for a description that creation would refuse, and for a mask that hides every object. */
int mcpt_compact_scene(const mcpt_scene_desc *desc, const uint8_t *visible /* n_objects */, mcpt_object *objects_out, mcpt_triangle *triangles_out,
                       int32_t *n_objects_out, int32_t *n_triangles_out, int32_t *prim_map /* n_triangles + n_objects entries */);

/* ---- Adding objects to a live scene: meshes, spheres and materials appended.
 *
 * mcpt_scene_add_objects appends the given objects, their triangles and the given materials to the scene's description and rebuilds the
 * traversal tree with the scene's own builder.  "Appended" is what mcpt_extend_scene computes: the objects after the existing ones in the
 * order given, the triangles after the existing ones with every first_tri shifted by the old triangle count, the materials after the
 * existing ones; environment and background untouched.  *first_object receives the index of the first added object (the old count).
 *   Ids: the triangles of existing objects keep their ids, the new triangles get n_triangles_old, n_triangles_old + 1, ...  A sphere's id
 *   is n_triangles + object, so the id of EVERY sphere, old or new, moves up by the number of added triangles -- which is what a fresh scene
 *   of the extended description reports.  Object indices never change.
 *   The added objects start without a transform and visible; the given triangles are their base, stored bit for bit.  Afterwards they are
 *   objects like any other to mcpt_scene_update, mcpt_scene_deform, mcpt_scene_set_materials and mcpt_scene_set_visibility.
 * THE CONTRACT: after the call every entry point listed at mcpt_scene_update gives what it gives on
 *       mcpt_scene_create_ex(compact(extend(desc', add)), device, the same options)
 * where desc' is the scene's current description (latest bases, current transforms, current materials), extend() is mcpt_extend_scene and
 * compact() is mcpt_compact_scene with the scene's current mask, in which the new objects are visible (ids translated as stated at
 * mcpt_scene_set_visibility).  Bit for bit with the host builders, the tree dump included; by the rule of mcpt_scene_update with the device
 * builders.  mcpt_scene_get_info equals the fresh scene's of extend(desc', add) in n_nodes, bvh_height, quantised, lds_resident, n_lights
 * and n_prims while nothing is hidden: lds_resident goes from 1 to 0 when the records outgrow what the LDS kernels hold.  A live scene
 * keeps the builder it was created with.
 * The handle, its streams and events, the wavefront workspaces and every mcpt_sequence made from the scene survive (a sequence holds no
 * primitive id and no array length of the scene).
 *   info->path 0  host: every host-built scene, and any scene when an added object emits light.  The extended description is flattened
 *                 and uploaded by the creation code, as path 0 of mcpt_scene_update.
 *   info->path 1  device: MCPT_BUILD_GPU_LBVH / MCPT_BUILD_GPU_PLOC scenes when no added object emits.  Record arrays of the new size are
 *                 allocated aside and the live records copied device to device (upload_ms); only the added triangles, a segment table and
 *                 the new material table cross the bus, and a kernel writes the records of the added primitives (transform_ms); the
 *                 device builder runs at the new size (build_ms).
 *   info->n_moved_tris is the number of added triangles.
 * Temporal reuse: when the scene has a snapshot (mcpt_scene_snapshot) it is extended in the same call with the added objects' records as
 * added, so they report zero object motion until the next snapshot, as if they had been there, at rest, when it was taken.
 * MCPT_ERR_ARG, before any device call: scene == NULL or add == NULL; a negative count; n_objects == 0; a non-zero reserved word; a null
 * array with a positive count; whatever creation refuses on the extended description (a triangle range out of bounds of add->triangles,
 * ranges that overlap, an object kind, material index or material type out of range); a vertex of an added triangle, a centre or a radius
 * that is not finite; totals (objects + triangles) beyond int32; a scene built with node instancing on.  A refused call, and a call whose
 * rebuild fails (MCPT_ERR_LIMIT: the new tree is deeper than the traversal stack; MCPT_ERR_OOM), leaves the scene exactly as it was, counts
 * and snapshot included: everything is built aside and swapped in as the last step.  Blocking, on the null stream, like mcpt_scene_update.
 * There is no removal: hide the object (mcpt_scene_set_visibility); removing it would renumber triangles. */
typedef struct {
    int32_t n_objects, n_triangles, n_materials;
    const mcpt_object   *objects;    /* first_tri is relative to `triangles` below; material indexes the table AFTER the append:
                                        0..M-1 the scene's entries, M..M+n_materials-1 the ones given here */
    const mcpt_triangle *triangles;
    const mcpt_material *materials;  /* appended to the material table; may be NULL with n_materials 0 */
    int32_t reserved[4];             /* must be 0 */
} mcpt_scene_addition;
int mcpt_scene_add_objects(mcpt_scene *scene, const mcpt_scene_addition *add, int32_t *first_object /* nullable */, mcpt_update_info *info /* nullable */);
/* Host only, no GPU needed: the description `desc` followed by the addition, which defines "appended".  Call it with the three arrays NULL
 * to get the counts, then with arrays of that size (materials_out included: the table is copied, then extended).  The environment and the
 * background stay the caller's.  MCPT_ERR_ARG for a null desc or add, for a description that creation would refuse, and for every
 * addition mcpt_scene_add_objects refuses. */
int mcpt_extend_scene(const mcpt_scene_desc *desc, const mcpt_scene_addition *add, mcpt_object *objects_out, mcpt_triangle *triangles_out,
                      mcpt_material *materials_out, int32_t *n_objects_out, int32_t *n_triangles_out, int32_t *n_materials_out);

/* Replaces the pixel/spp loop of Renderer::Render (Renderer.cpp:21-91): fb_host = W*H*3 floats,
 * row-major m = j*W + i, linear radiance averaged over spp -- what `framebuffer` holds at Renderer.cpp:91.
 * Blocking.  Tone map and PNG output (Renderer.cpp:95-109) stay with the caller. */
int mcpt_render(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, float *fb_host,
                mcpt_stats *stats);

/* Same, with the framebuffer left in HBM (fb_device: W*H*3 floats on the scene's device) and all work issued
 * on `hip_stream` (a hipStream_t; NULL = default stream).  Used when the caller reduces frames with RCCL. */
int mcpt_render_device(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, float *fb_device,
                       void *hip_stream, mcpt_stats *stats);

/* ---- Adaptive sampling.  Levels S0, 2 S0, 4 S0, ..., params.spp with S0 = opts.min_spp >= 2 and params.spp = S0 * 2^R, 0 <= R <= 15.
 * Round 0 renders every owned pixel at S0.  After each round every pixel active in it (n samples so far) is evaluated in double, in
 * exactly this order, s1 / s2 being the sums of v and v*v over its samples in sample order, v = (double) the float sample value:
 *     for c in 0..2:  m = s1[c]/n;  q = s2[c]/n - m*m;  var = max(q, 0) * n / (n - 1);  e_c = sqrt(var / n) / (m + rel_floor)
 *     e = max(e_0, e_1, e_2)            (NaN if any e_c is NaN; max(q, 0) keeps a NaN q; rel_floor and threshold widened to double)
 *     continue  iff  (e > threshold  or  (dilate and some 8-neighbour active in this round has e > threshold))  and  2n <= params.spp
 * A NaN estimate stops the pixel.  A continuing pixel's value is scaled by 0.5 and it gets samples [n, 2n), divisor 2n: halving is exact
 * (outside the subnormal range), so EVERY PIXEL IS BIT-IDENTICAL TO THE SAME PIXEL OF mcpt_render AT ITS FINAL SAMPLE COUNT.  Pixels the
 * sky cull finishes are final at S0 (their estimate is reported; they are not "active" for dilation).  Unowned pixels
 * (tile_size / rank / nranks) are 0 in every output.
 *   fb_host   W*H*3 floats, as mcpt_render
 *   spp_host  W*H final sample counts (nullable)
 *   err_host  W*H estimates e at the final counts: the rule is evaluated once more at params.spp, so capped pixels report one (nullable)
 *   info      rounds run, active pixels per round (round 0: every owned pixel), wall time per round (nullable)
 *   stats     sums over all rounds; samples = the sum of spp_host over owned pixels (nullable)
 * MCPT_ERR_ARG: params.spp not S0 * 2^R, S0 < 2, a negative or non-finite threshold, rel_floor <= 0, dilate not 0 or 1, or a non-zero
 * accumulate / spp_total / sample_offset.  MCPT_ERR_OVERFLOW as mcpt_render (the outputs are still written). */
typedef struct {
    int32_t min_spp;   /* S0 */
    int32_t dilate;    /* 0 | 1 */
    float threshold;   /* relative standard error of the mean that stops a pixel */
    float rel_floor;   /* added to the mean in the denominator */
    int32_t reserved[4];
} mcpt_adaptive; /* 32 bytes */
typedef struct {
    int32_t rounds;
    int32_t reserved;
    uint64_t active_pixels[16];
    double ms_round[16];
} mcpt_adaptive_info; /* 264 bytes */
int mcpt_render_adaptive(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, const mcpt_adaptive *opts,
                         float *fb_host, int32_t *spp_host, float *err_host, mcpt_adaptive_info *info, mcpt_stats *stats);

/* mcpt_render_adaptive with a per-pixel guide and the variance of the frame.  The rule above, with one change: pixel m's mark is
 *     e > threshold * sqrt((double) g),   g = guide_host[m] if guide_host[m] >= 1, otherwise g = 1
 * (the product and the square root in double), so a NaN, zero or negative guide leaves the plain rule, and so does a null guide_host.
 * The guide is meant to be the history length the pixel is about to get in a temporal blend (mcpt_temporal_history_len): a running mean
 * of N frames of equal variance has relative error e / sqrt(N), so the threshold becomes a target for the ACCUMULATED pixel.  err still
 * reports the unscaled e.  Dilation, sky-culled pixels, halving and the cap are unchanged, so every pixel is still bit-identical to the
 * same pixel of mcpt_render at its final count, and no pixel gets more samples than without the guide.
 *   guide_host     W*H floats (nullable: mcpt_render_adaptive's fb, spp and err bit for bit; an all-ones guide gives them too)
 *   variance_host  W*H floats (nullable): the luminance variance of the mean, step 2 of mcpt_render_denoised with n = the pixel's own
 *                  final count:  for c in 0..2:  m = s1/n;  q = s2/n - m*m;  var_c = max(q, 0) * n / (n - 1) / n;  v = sum_c w_c^2 var_c,
 *                  s1 / s2 the pixel's sums over all its samples; 0 for an unowned pixel (count 0)
 * MCPT_ERR_ARG and MCPT_ERR_OVERFLOW as mcpt_render_adaptive. */
int mcpt_render_adaptive_guided(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, const mcpt_adaptive *rule,
                                const float *guide_host, float *fb_host, int32_t *spp_host, float *err_host, float *variance_host,
                                mcpt_adaptive_info *info, mcpt_stats *stats);

/* mcpt_render_adaptive_guided with the weight mode of the guide: the plane holds, per pixel, the HISTORY WEIGHT H the pixel is about to
 * get in a weighted blend (mcpt_temporal_history_weight below): the samples behind its history.  With n samples so far pixel m's mark is
 *     e > threshold * sqrt((double) g),   g = (min(H, (max_history - 1) * n) + n) / n in float  if H > 0,  otherwise g = 1
 * (a zero, negative or NaN weight leaves the plain rule).  g is exactly the Neff the weighted blend will use if the pixel stops at n
 * samples (mcpt_temporal_accumulate_weighted, step 5 with s = n), so the threshold is a target for the ACCUMULATED pixel whatever the
 * counts of its earlier frames were; g >= 1, and it does not increase when n doubles, so a pixel's threshold tightens as it goes on.
 * err still reports the unscaled e.  The rule, halving, dilation and the cap are otherwise unchanged: every pixel is still bit-identical
 * to the same pixel of mcpt_render at its final count, and no pixel gets more samples than without the guide.
 *   history_weight_host  W*H floats (nullable: mcpt_render_adaptive_guided with a null guide, bit for bit)
 *   max_history          the cap of the blend the weights are meant for: 0 => 32; 1..4096 (mcpt_temporal_opts)
 * MCPT_ERR_ARG and MCPT_ERR_OVERFLOW as mcpt_render_adaptive_guided; MCPT_ERR_ARG also for max_history out of range. */
int mcpt_render_adaptive_weighted(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, const mcpt_adaptive *rule,
                                  const float *history_weight_host, int32_t max_history, float *fb_host, int32_t *spp_host, float *err_host,
                                  float *variance_host, mcpt_adaptive_info *info, mcpt_stats *stats);

/* ---- Feature buffers (AOVs) and a variance-guided a-trous denoiser (Dammertz et al. 2010; variance guidance of SVGF, Schied et al. 2017).
 *
 * AOV record: 8 floats per pixel, row-major m = j*W + i:  {albedo r,g,b, normal x,y,z, depth, coverage}.
 * Feature sample k of pixel m is EXACTLY the camera ray of render sample k (Philox key (seed, m), camera stream; mcpt_camera_rays),
 * traced with the scene's closest-hit traversal (mcpt_intersect) for every pixel (no sky cull).  Per sample:
 *   albedo    conductors: the reflectance of the hit, the checkerboard included (Material.hpp:134-151); dielectrics, emitters and misses: 1
 *   normal    the shading normal (the triangle's normal, or normalized(p - c) of a sphere), flipped to face the ray (dot(n, d) > 0 ? -n : n);
 *             a miss: 0
 *   depth     (float) of the double hit distance t;  coverage: 1 for a hit, 0 for a miss
 * Folded per pixel in sample order, in float: albedo and normal acc += v_k / aov_spp (normals are NOT renormalised: a silhouette pixel
 * carries a shorter one); depth = (sum of t_k over the hits) / hits, 0 without a hit; coverage = hits / aov_spp.
 *
 * Filter, in float32 (csrc/mcpt_denoise.h has every expression in its order; the device and a CPU build of it agree bit for bit):
 *   1. demodulate: A = max(albedo, 1e-3) per channel, e = colour / A; the variance input (the luminance variance of the colour mean)
 *      becomes v / lum(A)^2, lum = 0.2126 r + 0.7152 g + 0.0722 b.  A pixel whose colour, variance, e or scaled variance is not finite,
 *      or whose variance is negative, passes through unchanged and has weight 0 as a neighbour (in the prefilter too).
 *   2. depth gradient grad z: central differences over covered in-image neighbours; one-sided when one is missing, 0 when both are.
 *   3. iteration i = 0 .. iterations-1, step s = 2^i: g_p = the 3x3 binomial (1,2,1)^2 prefilter of v over the usable in-image neighbours
 *      on p's surface (both uncovered, or both covered with n_p.n_q > 0: the pairs whose tap weight below can be non-zero), normalised by
 *      the weights it used, so that not even the variance crosses a coverage seam or a seam of orthogonal normals; taps q = p + s (dx, dy),
 *      dy = -2..2, dx = -2..2 in that order, outside taps skipped:
 *          w = h(dx) h(dy) max(0, n_p.n_q)^sigma_n exp(-( |z_p - z_q| / (sigma_z |grad z_p . (s dx, s dy)| + 1e-3 max(z_p, z_q) + 1e-6)
 *                                                       + |l_p - l_q| / (sigma_l sqrt(g_p) + 1e-6) ))
 *      h = (1/16, 1/4, 3/8, 1/4, 1/16), l = lum(e).  Exactly one of cov_p, cov_q zero: w = 0; both zero: normal and depth terms are 1.
 *      e'_p = sum (w / sum w) e_q;  v'_p = sum (w / sum w)^2 v_q  (sum w e_q / sum w and sum w^2 v_q / (sum w)^2 in a form that keeps
 *      its precision: the weights of an edge pixel with a short folded normal can be subnormal); a pixel whose weights sum to 0 keeps its
 *      values.
 *      ^sigma_n by square-and-multiply with the integer sigma_n; exp is the library's own plain-IEEE exp (within 1 ulp; 0 below -87).
 *   4. remodulate: out = e * A.
 * MCPT_ERR_ARG for null pointers that are not nullable, width or height <= 0 and out-of-range options (a non-zero reserved word included). */
typedef struct {
    int32_t aov_spp;     /* feature samples per pixel; 0 => min(4, params.spp) (mcpt_render_denoised; mcpt_denoise ignores it) */
    int32_t iterations;  /* a-trous passes, step 2^i for i = 0..iterations-1; 0 => 5; at most 8 */
    float sigma_l;       /* luminance weight, > 0; 0 => 4 */
    float sigma_n;       /* normal exponent, an integer 1..1024; 0 => 128 */
    float sigma_z;       /* depth weight, > 0; 0 => 1 */
    int32_t specular_depth; /* delta bounces a feature sample follows, 0..8 (mcpt_render_aovs_ex); 0 => the first-hit AOVs
                               (mcpt_render_denoised; mcpt_denoise range-checks it and ignores it) */
    int32_t reserved[2]; /* must be 0 */
} mcpt_denoise_opts;     /* 32 bytes */

typedef struct { double ms_render, ms_aov, ms_denoise, ms_total; } mcpt_denoise_info; /* 32 bytes: HIP-event times of the stages, host wall time */

/* The AOV record of every pixel (aov_host: W*H*8 floats) for feature samples 0 .. aov_spp-1 of `seed`; aov_spp 0 => 4, at most 65536. */
int mcpt_render_aovs(mcpt_scene *scene, const mcpt_camera *camera, uint32_t seed, int32_t aov_spp, float *aov_host);

/* Feature samples that see through mirrors and glass.  specular_depth, 0..8, is the largest number of delta (Dirac) bounces one feature
 * sample follows.  Feature sample k of pixel m starts from the camera ray of render sample k (as above) with thr = (1,1,1) (float),
 * tsum = 0 (double) and a bounce count b = 0, then repeats:
 *   1. trace the closest hit of the current ray (d) with the scene's closest-hit traversal (mcpt_intersect);
 *   2. a miss: the sample records albedo thr, normal 0, coverage 0 and no depth; stop;
 *   3. a hit: tsum += t (the double hit distance); the hit point p = o + d * (float) t, the unflipped shading normal n, the uv and the
 *      material as for the first-hit AOVs above (and as the shading kernel forms them);
 *   4. if b < specular_depth, the material is Dirac (smooth conductor or smooth dielectric) and the hit is not an emitter, follow the
 *      bounce with the shading kernel's expressions at that vertex (Scene.cpp:109-159; mfn = n, what Material::sample returns for a smooth
 *      material), in channel 1 wherever an expression needs a channel:
 *        kr = fresnel(d, n, channel 1);  isReflect = kr > 0.5 (the more likely branch: always for conductors, kr = 1, and under total
 *        internal reflection);  wo = -d;
 *        p2 = isReflect ? (dot(wo, n) < 0 ? p - n*EPS : p + n*EPS) : (dot(wo, n) < 0 ? p + n*EPS : p - n*EPS)   (EPS = 1e-4f);
 *        wi = isReflect ? reflect(wo, n) : refract(d, n, channel 1);
 *        conductors: thr[c] *= eval(wi, wo, n, c, uv, isReflect = 1) for c = 0, 1, 2 (the weight the render gives that mirror bounce
 *        in that channel, the checkerboard included); dielectrics leave thr unchanged;
 *      then b += 1 and the next ray is (p2, wi): back to 1;
 *   5. otherwise the sample records this hit: albedo = thr[c] * the first-hit albedo of this hit (above), normal = this hit's n flipped
 *      to face the ray that reached it, depth = (float) tsum, coverage 1.
 * The samples are folded per pixel exactly as above.  The direction follows channel 1 of a dispersive material; the colour frame, its
 * Philox streams and fb are untouched.  specular_depth 0 gives exactly mcpt_render_aovs (1 * x = x and (float) tsum = (float) t), and the
 * call then runs the first-hit kernels themselves.  MCPT_ERR_ARG as mcpt_render_aovs, and for specular_depth outside 0..8, before any
 * device call. */
int mcpt_render_aovs_ex(mcpt_scene *scene, const mcpt_camera *camera, uint32_t seed, int32_t aov_spp, int32_t specular_depth, float *aov_host);

/* The filter on host arrays: color_host W*H*3, variance_host W*H (luminance variance of each colour mean), aov_host W*H*8 (as
 * mcpt_render_aovs), out_host W*H*3.  The scene only picks the device and stream, as in mcpt_tonemap. */
int mcpt_denoise(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *variance_host, const float *aov_host,
                 const mcpt_denoise_opts *opts, float *out_host);

/* mcpt_render, then the filter, on one stream:
 *   1. the frame with the per-pixel moments of adaptive round 0 (mcpt_render_adaptive): fb_host is BIT-IDENTICAL to mcpt_render's frame
 *      (sky-culled pixels take their moments from the constant background samples);
 *   2. the luminance variance of the mean, in double, rounded once to float, n = params.spp, w = (0.2126, 0.7152, 0.0722):
 *          for c in 0..2:  m = s1/n;  q = s2/n - m*m;  var_c = max(q, 0) * n / (n - 1) / n;   v = sum_c w_c^2 var_c
 *      It ignores the covariance between the channels: the R, G and B paths are separate Philox streams and share only the camera ray;
 *   3. the AOVs of mcpt_render_aovs_ex(params.seed, opts.aov_spp, opts.specular_depth);  4. mcpt_denoise of the three.
 * So fb, variance and aov are what the separate calls return, and denoised equals mcpt_denoise(fb, variance, aov, opts) bit for bit.
 *   fb_host, denoised_host  W*H*3 floats;  variance_host W*H floats (nullable);  aov_host W*H*8 floats (nullable);  info (nullable);
 *   stats as mcpt_render (nullable).
 * MCPT_ERR_ARG also for params.spp < 2, opts.aov_spp > params.spp, nranks != 1, or a non-zero accumulate / spp_total / sample_offset
 * (a partial or partitioned frame is not denoised).  MCPT_ERR_OVERFLOW as mcpt_render (the outputs are still written). */
int mcpt_render_denoised(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, const mcpt_denoise_opts *opts, float *fb_host,
                         float *denoised_host, float *variance_host, float *aov_host, mcpt_denoise_info *info, mcpt_stats *stats);

/* An adaptive frame, then the filter, on one stream:
 *   mcpt_render_adaptive_guided(rule, guide_host) with its variance;  the AOVs of mcpt_render_aovs_ex(params.seed, opts.aov_spp,
 *   opts.specular_depth);  mcpt_denoise of the three.
 * fb, spp, err, variance and aov are what the separate calls return and denoised equals mcpt_denoise(fb, variance, aov, opts), bit for bit.
 * The filter gets each pixel's own variance: a pixel that stopped early carries the larger one and is smoothed more.
 *   guide_host nullable;  fb_host, denoised_host W*H*3;  spp_host, err_host, variance_host W*H, aov_host W*H*8 (each nullable);
 *   adaptive_info, info, stats nullable (info.ms_render is the time of the rounds).
 * MCPT_ERR_ARG: every case of mcpt_render_adaptive and of mcpt_render_denoised (params.spp >= 2, nranks == 1), and opts.aov_spp >
 * rule.min_spp -- every pixel has at least min_spp samples and feature sample k is render sample k; aov_spp 0 => min(4, min_spp). */
int mcpt_render_adaptive_denoised(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_params *params, const mcpt_adaptive *rule,
                                  const float *guide_host, const mcpt_denoise_opts *opts, float *fb_host, float *denoised_host,
                                  int32_t *spp_host, float *err_host, float *variance_host, float *aov_host,
                                  mcpt_adaptive_info *adaptive_info, mcpt_denoise_info *info, mcpt_stats *stats);

/* ---- Temporal reuse for moving scenes: per-pixel motion and a validated blend of the reprojected history (csrc/mcpt_temporal.h has
 * every expression in its order; the device and a CPU build of it agree bit for bit).  The frame loop is
 *       mcpt_scene_snapshot;  mcpt_scene_update;  mcpt_render (+ mcpt_render_aovs);  mcpt_render_motion;  mcpt_temporal_blend.
 * (mcpt_sequence_frame below runs that loop on the device, with the variance of the accumulated frame and the filter.)
 *
 * mcpt_scene_snapshot remembers where the geometry is now: the live triangle records (v0, e1, e2) and sphere centres are copied device to
 * device into arrays the scene owns (allocated on first use, reallocated only if the counts change, freed by mcpt_scene_destroy).
 * Primitive ids are stable across mcpt_scene_update, so entry p of the snapshot is primitive p, however many updates follow it.  A scene
 * that was never snapshotted uses its live arrays as "previous" (camera motion only).  MCPT_ERR_ARG for a null scene; MCPT_ERR_OOM leaves
 * the old snapshot intact. */
int mcpt_scene_snapshot(mcpt_scene *scene);

/* Motion record: 4 floats per pixel, row-major m = j*W + i:  {dx, dy, prev_depth, valid}.
 * Feature sample k of pixel m is the camera ray of render sample k, traced exactly as for mcpt_render_aovs (same keys, same closest-hit
 * traversal, no sky cull).  Per hit sample, in float unless stated:
 *   triangle  (u, v) = the double barycentrics of the hit on the live record, each rounded once to float;
 *             p_cur = v0 + (e1*u + e2*v) on the live record, p_prev = the same expression on the snapshot's record
 *             (a static triangle gives p_prev == p_cur bit for bit)
 *   sphere    p_cur = o + d * (float) t;  p_prev = p_cur + (c_prev - c_cur)   (the linear part of a transform acts on the centre only)
 *   proj(cam, p):  q = orientation^T (p - position), each component in the 3-term dot order a.x*b.x + (a.y*b.y + a.z*b.z);
 *             invalid if q.z <= 0;  sx = (1 - (q.x/q.z)/(aspect*scale)) * (0.5f*W),  sy = (1 - (q.y/q.z)/scale) * (0.5f*H)
 *             with the scale = tan(fov/2) and aspect = W/H of the camera rays: the inverse of their x, y through a pinhole at `position`
 *             (the lens offset of a depth-of-field camera is ignored), in pixels, pixel i covering [i, i+1)
 *   motion    proj(prev_camera, p_prev) - proj(camera, p_cur): 0 bit for bit when nothing moved; the pixel jitter and the lens sample
 *             cancel to first order
 *   prev_depth  |p_prev - prev_camera.position|: the 3-term dot of the difference with itself, then sqrtf
 *   A sample is invalid if it misses or if either projection has q.z <= 0.  A point that leaves the previous frustum sideways stays
 *   valid: being off-screen is the blend's business.
 * Folded per pixel in sample order: dx, dy and prev_depth are each the sum over the valid samples divided by their number (0 without
 * one); valid = that number / aov_spp.
 * motion_host: W*H*4 floats.  aov_spp 0 => 4, at most 65536.  MCPT_ERR_ARG, before any device call: a null pointer, width or height
 * <= 0, aov_spp out of range, prev_camera with another width or height than camera.
 * Limits: the motion is that of the first hit, so what is seen through mirrors and glass is not reprojected (mcpt_render_motion_ex below
 * does that), nor is depth-of-field blur. */
int mcpt_render_motion(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_camera *prev_camera, uint32_t seed, int32_t aov_spp,
                       float *motion_host);

/* The motion of what is seen through mirror and glass chains (csrc/mcpt_specular_motion.h has every expression in its order).
 * specular_depth 0: mcpt_render_motion, bit for bit (the same kernels).  Otherwise feature sample k of pixel m walks exactly the chain of
 * mcpt_render_aovs_ex(seed, aov_spp, specular_depth): the same camera ray, closest-hit traversal, stop rule (fewer than specular_depth
 * bounces so far, a Dirac material, not an emitter), branch (kr = fresnel of channel 1, reflect iff kr > 0.5), next origin and direction --
 * one device function decides the bounce for both passes.  A sample carries two affine maps of R^3, A_cur and A_prev (3 x 4 floats each),
 * both "none" at the start; all arithmetic in float, no contraction, dots in the 3-term order:
 *   followed reflect bounce  one mirror plane per map, anchor a and unit normal n (the sign of n does not matter):
 *             triangle  (u, v) as above;  a_cur = v0 + (e1*u + e2*v) on the live record, a_prev the same on the snapshot's;  n = the unit
 *                       normal derived from that record's own e1, e2: c = cross(e1, e2), z = c.c, n = z > 0 ? c / sqrtf(z) : c
 *                       (equal records give equal normals bit for bit)
 *             sphere    a_cur = o + d * (float) t,  a_prev = a_cur + (c_prev - c_cur),  n_cur = n_prev = normalized(a_cur - c_cur)
 *             R(a, n)(x) = x - 2 n (n . (x - a)), as the map L = I - (2n) n^T, t = (2n)(n . a);  A <- A o R, so that the newest reflection
 *             is applied first: v = R1(R2(... Rk(q)))
 *   followed refract bounce  both maps stay as they are: glass is treated as straight-through
 *   terminal hit (the vertex where the chain AOVs record)  q_cur, q_prev = p_cur, p_prev of the rule above on the last ray and its hit;
 *             v_cur = A_cur(q_cur), v_prev = A_prev(q_prev), a map that is still none not applied (v = q bit for bit);  the record is that
 *             of the points v_cur, v_prev: motion = proj(prev_camera, v_prev) - proj(camera, v_cur), prev_depth = |v_prev - prev position|
 *   a chain that ends in a miss: an invalid sample.  The fold is unchanged.
 * v is the *virtual point*: the terminal hit reflected back across the mirror planes the chain passed, which lies on the primary ray at
 * about the chain's depth (channel 6 of the chain AOVs).  For planar mirrors that is exact under any rigid motion of object, mirror and
 * camera; for a curved mirror (the tangent plane at the hit) and for refraction it is the usual approximation, and the depth test of
 * the blend, against the chain depth of the previous frame, decides whether the history is usable.  So:
 *   - equal cameras and a snapshot equal to the live geometry give dx = dy = 0 bit for bit (the same expressions on the same inputs);
 *   - valid equals the coverage channel of the chain AOVs whenever both projections have q.z > 0.
 * MCPT_ERR_ARG, before any device call: as mcpt_render_motion, and specular_depth outside 0..8.
 * Limits: depth-of-field blur is not reprojected; refraction and curved mirrors as said. */
int mcpt_render_motion_ex(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_camera *prev_camera, uint32_t seed, int32_t aov_spp,
                          int32_t specular_depth, float *motion_host);

/* The blend on host arrays (the scene only picks the device and stream, as in mcpt_denoise):
 *   color_host W*H*3 the new frame;  motion_host W*H*4 (mcpt_render_motion);  prev_color_host W*H*3 the previous OUTPUT of this call;
 *   prev_depth_host W*H the depth channel of the previous frame's AOVs;  prev_len_host / out_len_host W*H floats with integer values:
 *   the number of frames already blended into a pixel (0 everywhere for the first frame);  out_color_host W*H*3.
 * Per pixel (i, j), in float, in this order:
 *   1. motion.valid <= 0, or a colour channel that is not finite: out = color, len = 1.
 *   2. fx = i + dx, fy = j + dy (pixel-centre coordinates minus 0.5);  x0 = floorf(fx), a = fx - x0;  y0 = floorf(fy), b = fy - y0;
 *      taps (x0,y0), (x0+1,y0), (x0,y0+1), (x0+1,y0+1) in that order with weights (1-a)(1-b), a(1-b), (1-a)b, ab.
 *   3. a tap is skipped if its weight is 0 (a static frame reads exactly one tap), it lies outside the image, prev_len <= 0 there, a
 *      channel of its colour is not finite, or |prev_depth[tap] - motion.prev_depth| > depth_tol * motion.prev_depth
 *      (tested as !(|..| <= ..), so a depth that is NaN on either side skips the tap too).
 *   4. no tap left: out = color, len = 1.
 *   5. otherwise, per channel, sums from 0 in tap order:  hist = (sum w c) / (sum w);  n = the smallest prev_len of the used taps;
 *      N = min(n + 1, max_history);  out = hist + (color - hist) * (1.f / N);  len = N.
 * So a static scene accumulates the running mean of its frames (N frames after N calls, up to max_history, then an exponential average),
 * and a pixel whose history fails the depth test restarts.  Only depth is validated: a rotating object keeps its history, and sky
 * pixels (valid 0) restart every frame.  (mcpt_temporal_accumulate_ex below adds a normal test and a colour clamp.)
 * MCPT_ERR_ARG for a null pointer, width or height <= 0 and out-of-range options (a non-zero reserved word included). */
typedef struct {
    int32_t max_history; /* cap of the running mean's length; 0 => 32; 1..4096 */
    float depth_tol;     /* relative depth tolerance, > 0; 0 => 0.02 */
    int32_t reserved[6]; /* must be 0 */
} mcpt_temporal_opts;    /* 32 bytes */
int mcpt_temporal_blend(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *motion_host,
                        const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host, const mcpt_temporal_opts *opts,
                        float *out_color_host, float *out_len_host);

/* The blend with the variance of its result, on host arrays: the testable form of the kernel a sequence runs, as mcpt_temporal_blend is
 * of its.  The arguments of mcpt_temporal_blend, and
 *   variance_host W*H  this frame's luminance variance of the colour mean (the `variance` of mcpt_render_denoised, step 2), v_c below;
 *   prev_variance_host W*H  the previous out_variance_host of this call;   out_variance_host W*H.
 * out_color and out_len are EXACTLY those of mcpt_temporal_blend on the same inputs: the same taps, skips, hist, N and out.  Per pixel:
 *   - where the blend takes no history (its steps 1 and 4):  out_variance = v_c;
 *   - otherwise, over the taps the colour used, in tap order and from 0, in float:
 *         sv = sv + (w*w) * prev_variance[tap];   hv = sv / (sw*sw)   (sw = the sum of w of step 5);
 *         k = 1.f / N;   omk = 1.f - k;   out_variance = (omk*omk)*hv + (k*k)*v_c
 *     -- the variance of hist + (color - hist)*k for independent terms: a static pixel carries (sum of its frames' variances) / N^2
 *     after N frames;
 *   - hv not finite or negative (a tap's stored variance was):  out_variance = v_c.  One frame's variance over-estimates that of the
 *     accumulated pixel, so a filter guided by it smooths more, never less;
 *   - a NaN v_c propagates (the filter passes such a pixel through unchanged).
 * Bilinear resampling correlates neighbouring output pixels (two that share a tap share its noise); the propagation ignores that
 * covariance, as it ignores the correlation of the taps themselves.
 * MCPT_ERR_ARG as mcpt_temporal_blend. */
int mcpt_temporal_accumulate(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                             const float *motion_host, const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host,
                             const float *prev_len_host, const mcpt_temporal_opts *opts, float *out_color_host, float *out_variance_host,
                             float *out_len_host);

/* History rejection: mcpt_temporal_accumulate with a normal test on every tap and a neighbourhood colour clamp of the reprojected
 * history, so that a crease does not mix the colours of its two faces and a change of lighting (a moved emitter or occluder, which
 * leaves the depth of the pixels it lights untouched) does not fade out over max_history frames.  The arguments of
 * mcpt_temporal_accumulate, and
 *   normal_host W*H*3  this frame's first-hit normals: channels 3..5 of the AOVs of mcpt_render_aovs (specular_depth 0), folded as they
 *                      are -- a mean of unit vectors, not renormalised;
 *   prev_normal_host W*H*3  the normal_host of the previous call;
 *   out_flags_host W*H bytes, nullable: bit 0 (1) the normal test skipped a tap, bit 1 (2) the clamp moved the history.
 * The rule is that of mcpt_temporal_blend / mcpt_temporal_accumulate with three additions, all in float, without contraction:
 *   step 3, one more skip, tested last (normal_test 1):  pn = prev_normal[tap], n = normal[p];
 *         d = pn.x*n.x + (pn.y*n.y + pn.z*n.z);   the tap is skipped if !(d >= normal_min)   (a NaN normal on either side skips it).
 *      Flag bit 0 is set when this test skipped at least one tap that every older test had passed and the pixel still takes history.
 *   after hist is formed in step 5 (color_clamp 1):  over the 3x3 neighbours q of p in the NEW frame `color` that lie inside the image, in
 *      the order dy = -1..1, then dx = -1..1, p itself included, using only those whose three channels are finite; n = their number
 *      (p is finite by step 1, so n >= 1), as a float.  Per channel, sums from 0 in that order:
 *         s = s + c;   s2 = s2 + c*c;   mu = s/n;   var = max(s2/n - mu*mu, 0);   sd = sqrtf(var);
 *         lo = mu - clamp_k*sd;   hi = mu + clamp_k*sd;   hist' = min(max(hist, lo), hi)
 *      with max(x, 0) = x > 0 ? x : 0 (0 for a NaN) and the clamp as two comparisons, t = hist < lo ? lo : hist;  hist' = t > hi ? hi : t,
 *      so a bound that is NaN (sums that overflowed) leaves hist as it is.  Then out = hist' + (color - hist') * (1.f / N);  len = N,
 *      unchanged: a clamped history still counts its frames.
 *   if any channel has hist' != hist:  flag bit 1 is set and out_variance = v_c -- the propagated variance describes a history that was
 *      not used as it was, and one frame's variance over-estimates, so the filter smooths more, never less.
 * Pixels that take no history (steps 1 and 4) have flags 0.  With both switches 0 the call gives mcpt_temporal_accumulate's outputs bit
 * for bit (it launches the same kernel), flags 0 everywhere, and normal_host / prev_normal_host are not read and may be null.
 * clamp_k: the default 1 is the smallest of 1, 1.5, 2, 3 whose cost on a static scene stays inside the seed-to-seed spread of the
 * unclamped error (DESIGN section 8f has the figures).
 * MCPT_ERR_ARG, before any device call: every case mcpt_temporal_accumulate refuses; a null history_opts; a switch that is not 0 or 1;
 * normal_min or clamp_k out of range or NaN (checked whether or not their switch is on); a non-zero reserved word; normal_test 1 with a
 * null normal_host or prev_normal_host. */
typedef struct {
    int32_t normal_test; /* 0 off, 1 on */
    int32_t color_clamp; /* 0 off, 1 on */
    float normal_min;    /* 0 => 0.9; otherwise in (0, 1] */
    float clamp_k;       /* 0 => 1; otherwise > 0 and finite */
    int32_t reserved[4]; /* must be 0 */
} mcpt_history_opts;     /* 32 bytes; a zeroed struct switches both tests off */
int mcpt_temporal_accumulate_ex(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                                const float *motion_host, const float *normal_host, const float *prev_color_host,
                                const float *prev_variance_host, const float *prev_depth_host, const float *prev_len_host,
                                const float *prev_normal_host, const mcpt_temporal_opts *opts, const mcpt_history_opts *history_opts,
                                float *out_color_host, float *out_variance_host, float *out_len_host, uint8_t *out_flags_host);

/* The history length every pixel is ABOUT TO GET, before its frame is rendered: steps 1-4 of the blend and the N of step 5, with the new
 * colour taken to be finite.  Per pixel, in float, in this order:
 *   motion.valid <= 0:  1;   otherwise the taps of step 2 with every skip of step 3, the normal test of mcpt_temporal_accumulate_ex
 *   included when history_opts.normal_test is 1;   no tap left:  1;   otherwise  N = min(n + 1, max_history), n the smallest prev_len of
 *   the used taps.
 * The colour clamp does not enter: a clamped history keeps its length.  Neither the new colour nor any variance is read.
 * So len_host[m] EQUALS THE out_len[m] OF mcpt_temporal_accumulate_ex ON THE SAME INPUTS FOR EVERY PIXEL WHOSE NEW COLOUR IS FINITE
 * (a pixel with a non-finite colour restarts there, len 1).  It is the guide of mcpt_render_adaptive_guided in a sequence.
 *   motion_host W*H*4;  prev_color_host W*H*3 (only its finiteness is read), prev_depth_host, prev_len_host W*H;  normal_host,
 *   prev_normal_host W*H*3, nullable unless normal_test is 1;  history_opts nullable (both switches off);  len_host W*H.
 * The scene only picks the device and stream.  MCPT_ERR_ARG, before any device call: as mcpt_temporal_accumulate_ex. */
int mcpt_temporal_history_len(mcpt_scene *scene, int32_t width, int32_t height, const float *motion_host, const float *normal_host,
                              const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host,
                              const float *prev_normal_host, const mcpt_temporal_opts *opts, const mcpt_history_opts *history_opts,
                              float *len_host);

/* The accumulation with the history weighted by sample counts: frames of a sequence whose pixels have different counts (adaptive frames, or
 * a params.spp that changes from frame to frame) weigh by their samples, not 1/N each.  For one pixel the per-sample variance is the same
 * from frame to frame, so counts are the inverse-variance weights up to a factor, and unlike an estimated variance they carry no noise of
 * their own into the weights.  The arguments of mcpt_temporal_accumulate_ex, and
 *   count_host W*H int32, nullable  the samples behind each pixel of this frame (the spp map of an adaptive frame);
 *   uniform_count                   used for every pixel when count_host is null (params.spp of a uniform frame);
 *   prev_weight_host W*H            the previous out_weight_host of this call (0 everywhere for the first frame);   out_weight_host W*H.
 * Per pixel s = (float) count[p], or uniform_count; s >= 1.  The rule of mcpt_temporal_accumulate_ex with three changes, all in float,
 * without contraction, in this order:
 *   step 3, one more skip, tested together with prev_len <= 0:  a tap is skipped if !(prev_weight[tap] > 0)  (a NaN weight skips it);
 *   step 5:  Hmin = the smallest prev_weight of the used taps (conservative, as n is for len);
 *         Hc = min(Hmin, (max_history - 1) * s);   Neff = (Hc + s) / s;   k = 1.f / Neff;
 *         out = hist + (color - hist) * k;   out_weight = Hc + s;
 *      len stays N = min(n + 1, max_history): it still counts frames; the flags and the depth, normal and clamp logic are untouched; the
 *      variance keeps its formula, (omk*omk)*hv + (k*k)*v_c with this k and omk = 1.f - k;
 *   a pixel that takes no history (steps 1 and 4) gets out_weight = s.
 * So a static pixel carries sum(s_k c_k) / sum(s_k) and the weight sum(s_k), and max_history caps the weight at max_history * s of the
 * current frame, as it caps len.  k is formed as 1.f / Neff and not as s / (Hc + s) on purpose: WITH UNIFORM COUNTS, prev_weight EQUAL TO
 * prev_len * s AND max_history * s < 2^24, Neff IS THE INTEGER N EXACTLY (every term is an integer below 2^24), SO out_color,
 * out_variance, out_len AND out_flags ARE THOSE OF mcpt_temporal_accumulate_ex BIT FOR BIT, AND out_weight = out_len * s.
 * MCPT_ERR_ARG, before any device call: every case mcpt_temporal_accumulate_ex refuses; a null prev_weight_host or out_weight_host; a
 * count below 1 anywhere in count_host (the array is scanned on the host); with a null count_host a uniform_count below 1 or not finite. */
int mcpt_temporal_accumulate_weighted(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                                      const float *motion_host, const float *normal_host, const int32_t *count_host, float uniform_count,
                                      const float *prev_color_host, const float *prev_variance_host, const float *prev_depth_host,
                                      const float *prev_len_host, const float *prev_normal_host, const float *prev_weight_host,
                                      const mcpt_temporal_opts *opts, const mcpt_history_opts *history_opts, float *out_color_host,
                                      float *out_variance_host, float *out_len_host, uint8_t *out_flags_host, float *out_weight_host);

/* The history weight every pixel is ABOUT TO GET, before its frame is rendered, as mcpt_temporal_history_len is for the length: steps 1-4
 * of mcpt_temporal_accumulate_weighted with the new colour taken to be finite -- the weight skip, and the normal test when
 * history_opts.normal_test is 1 -- and the Hmin of step 5; 0 where the pixel takes no history.  Neither colour nor variance is read.
 * So FOR EVERY PIXEL WHOSE NEW COLOUR IS FINITE  out_weight == min(weight, (max_history - 1) * s) + s  OF
 * mcpt_temporal_accumulate_weighted ON THE SAME INPUTS.  It is the guide of mcpt_render_adaptive_weighted in a sequence.
 * The arguments of mcpt_temporal_history_len, and prev_weight_host W*H;  weight_host W*H.
 * MCPT_ERR_ARG, before any device call: as mcpt_temporal_history_len; a null prev_weight_host or weight_host. */
int mcpt_temporal_history_weight(mcpt_scene *scene, int32_t width, int32_t height, const float *motion_host, const float *normal_host,
                                 const float *prev_color_host, const float *prev_depth_host, const float *prev_len_host,
                                 const float *prev_normal_host, const float *prev_weight_host, const mcpt_temporal_opts *opts,
                                 const mcpt_history_opts *history_opts, float *weight_host);

/* ---- Frame sequences: the history, the variance of the accumulated frame and every working buffer stay on the device; one call runs a
 * whole frame on one stream and only what the caller asks for crosses the bus.  The caller's loop is
 *       mcpt_scene_update;  mcpt_sequence_frame          (params.seed varied from frame to frame).
 *
 * mcpt_sequence_create allocates everything once, per pixel: two history sets (colour 3, variance 1, depth 1, len 1 floats, used in
 * turn), the frame 3, its moments 6 doubles, its variance 1, the AOVs 8 (8 more with denoise.specular_depth > 0), the motion 4, the
 * filtered frame 3 and the tone-mapped one (4 bytes), and the filter's working buffers (72 bytes): 248 bytes per pixel.  It also takes
 * the scene's snapshot (mcpt_scene_snapshot).  A failed allocation frees what it had: MCPT_ERR_OOM.  mcpt_sequence_frame allocates
 * nothing of its own (the wavefront workspace is the scene's, sized by its first render as in mcpt_render).
 * THE SEQUENCE OWNS THE SCENE'S SNAPSHOT WHILE IT LIVES: every frame ends with mcpt_scene_snapshot, so that this frame's geometry is
 * "previous" for the next one; a caller that snapshots the scene itself changes what the next frame's motion refers to.  One sequence per
 * scene at a time.  The sequence borrows the scene: destroy the sequence first; destroying the scene first is the caller's error.
 *
 * mcpt_sequence_frame, in this order on one stream:
 *   1. the checks of mcpt_render_denoised on (camera, params, opts.denoise): params.spp >= 2, nranks == 1, accumulate / spp_total /
 *      sample_offset 0, denoise.aov_spp <= params.spp; and camera.width / height must be the sequence's;
 *   2. the frame with its moments and its variance: steps 1-2 of mcpt_render_denoised (fb is BIT-IDENTICAL to mcpt_render's frame);
 *   3. the AOVs of mcpt_render_aovs_ex(params.seed, denoise.aov_spp, denoise.specular_depth).  The history is always validated against
 *      FIRST-HIT depth, which is what a motion record's prev_depth measures: with specular_depth 0 that is the depth channel of these AOVs,
 *      otherwise one more first-hit pass (specular_depth 0, the same aov_spp) supplies it;
 *   4. the motion of mcpt_render_motion(camera, the camera of the sequence's previous frame, params.seed, denoise.aov_spp) against the
 *      scene's snapshot; the first frame, and the first frame after a reset, use this frame's camera as the previous one;
 *   5. mcpt_temporal_accumulate(frame, variance, motion, the history: colour, variance, first-hit depth, len; opts.temporal) from the
 *      previous history set into the other, which also receives this frame's first-hit depth.  On the first frame and after a reset
 *      prev_len is 0 everywhere, so every pixel starts;
 *   6. opts.filter 1: mcpt_denoise(accumulated, the accumulated variance, the AOVs; opts.denoise).  The filter gets the variance of the
 *      image it filters.  The history stays unfiltered: the filter is an output, not a feedback -- unless the sequence was created
 *      with mcpt_sequence_create_feedback (below), which feeds the filter's iteration k back into the history;
 *   7. the tone map (mcpt_tonemap) if rgba was asked for; then the downloads;
 *   8. mcpt_scene_snapshot.
 * So every output equals what the separate calls give on the same inputs, bit for bit.
 * mcpt_sequence_outputs: host pointers, each nullable; a null pointer costs no download (a null struct pointer: none at all).
 * mcpt_sequence_info: HIP-event times of the stages, the host wall time, and the index of this frame since the last reset (0 for the
 * first).  stats as mcpt_render (nullable).
 * mcpt_sequence_reset is a camera cut: the next frame takes no history (len 1, accumulated == fb, variance == the frame's own).
 * MCPT_ERR_OVERFLOW as mcpt_render: the outputs are still written and the history is still advanced.  Any other failure leaves the
 * history, the frame index and the remembered camera as they were before the call.
 * MCPT_ERR_ARG, before any device call: a null scene, sequence, camera, params, opts or out; width or height <= 0 or a frame too
 * large; out-of-range temporal or denoise options, a non-zero reserved word; filter not 0 or 1; the failed checks of step 1;
 * outputs.denoised non-null with filter 0. */
typedef struct {
    mcpt_temporal_opts temporal;
    mcpt_denoise_opts denoise;
    int32_t filter;      /* 0: accumulate only (what a zeroed struct asks for); 1: also filter the accumulated frame */
    int32_t reserved[7]; /* must be 0 */
} mcpt_sequence_opts;    /* 96 bytes */
typedef struct {
    float *fb;           /* this frame, W*H*3 */
    float *accumulated;  /* the accumulated frame, W*H*3 */
    float *denoised;     /* the filtered accumulated frame, W*H*3 (filter 1 only) */
    float *variance;     /* W*H, of the accumulated frame */
    float *len;          /* W*H */
    float *aov;          /* W*H*8 */
    float *motion;       /* W*H*4 */
    uint8_t *rgba;       /* W*H*4 bytes: mcpt_tonemap of denoised, or of accumulated when filter is 0 */
} mcpt_sequence_outputs; /* 64 bytes */
typedef struct {
    double ms_render, ms_aov, ms_motion, ms_accumulate, ms_filter; /* HIP-event times; ms_filter includes the tone map */
    double ms_total;     /* host wall time of the call */
    int32_t frame_index; /* frames since the last reset, this one not counted */
    int32_t reserved[3];
} mcpt_sequence_info;    /* 64 bytes */
typedef struct mcpt_sequence mcpt_sequence;
int mcpt_sequence_create(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts, mcpt_sequence **out);
int mcpt_sequence_frame(mcpt_sequence *sequence, const mcpt_camera *camera, const mcpt_params *params, const mcpt_sequence_outputs *outputs,
                        mcpt_sequence_info *info, mcpt_stats *stats);
int mcpt_sequence_reset(mcpt_sequence *sequence);
void mcpt_sequence_destroy(mcpt_sequence *sequence);

/* A sequence with history rejection (mcpt_history_opts above).  A null or zeroed history_opts: mcpt_sequence_create, exactly.  Otherwise
 * step 5 of mcpt_sequence_frame is mcpt_temporal_accumulate_ex in place of mcpt_temporal_accumulate, and every output still equals what
 * the separate calls give, bit for bit:
 *   normal_test 1: each history set gains a normal plane (3 floats per pixel), which step 5 writes from channels 3..5 of the first-hit
 *      AOVs -- the AOVs the depth plane comes from: those of step 3 with denoise.specular_depth 0, otherwise the extra first-hit pass;
 *   either switch 1: each history set gains a flags plane (1 byte per pixel), which step 5 writes.
 * Per pixel that is 24 bytes more with normal_test and 2 more with either switch: up to 274 with both (306 with specular_depth > 0).
 * mcpt_sequence_flags copies the flags of the last successful frame to flags_host (W*H bytes; all 0 before the first frame).  A failed
 * frame leaves history, normals and flags as they were; mcpt_sequence_reset leaves the flags of the last frame readable.
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create and mcpt_temporal_accumulate_ex; mcpt_sequence_flags for a null pointer
 * or a sequence created with both switches 0 (it keeps no flags). */
int mcpt_sequence_create_ex(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts, const mcpt_history_opts *history_opts,
                            mcpt_sequence **out);
int mcpt_sequence_flags(mcpt_sequence *sequence, uint8_t *flags_host);

/* A sequence whose frames are adaptive, the stopping threshold relaxed by the history each pixel is about to have.  A null `adaptive`:
 * mcpt_sequence_create_ex, exactly (the same allocations, the same frame).  Otherwise mcpt_sequence_frame takes params.spp as the CAP of
 * the rule: step 1 also checks params.spp == rule.min_spp * 2^R (0 <= R <= 15) and denoise.aov_spp <= rule.min_spp (aov_spp 0 =>
 * min(4, min_spp)), and the frame runs on one stream in this order:
 *   a. the AOVs (step 3), and the first-hit pass when specular_depth > 0;   b. the motion (step 4) -- neither depends on the frame, so
 *      moving them in front changes no output;
 *   c. guided 1: the guide = mcpt_temporal_history_len(motion, the first-hit normals, the previous history set: colour, depth, len,
 *      normals; opts.temporal, history_opts).  On the first frame and after a reset prev_len is 0, so the guide is 1 everywhere;
 *   d. the rounds of mcpt_render_adaptive_guided(rule, the guide; guided 0: no guide) and its variance, each pixel at its own count;
 *   e. steps 5-8 as they are: the history and the filter get each pixel's own variance.  A pixel's frames weigh 1/N each in the blend,
 *      whatever their counts, unless the sequence is weighted (mcpt_sequence_create_weighted below weighs them by their counts).
 * outputs.fb is the adaptive frame; every output equals what the separate calls give, bit for bit.  stats.samples is the sum of the
 * count map.  In mcpt_sequence_info the guide is counted with ms_motion and ms_render is the time of the rounds.
 * Allocated at create, for all W*H pixels active, per pixel: two sets of counts (spp 4, err 4, guide 4 bytes, used in turn with the
 * history sets), the stamps 1, both lists 4 + 4 with their candidate entries 16 + 16, the flags 1: 66 bytes per pixel, plus the
 * compaction's scratch (a few KiB).  A frame allocates nothing.
 * mcpt_sequence_counts copies the counts, the estimates and the guide (0 everywhere without guided) of the last
 * successful frame, each pointer nullable (all 0 before the first frame); a failed frame leaves history, counts and guide as they were.
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_ex; min_spp < 2, a negative or non-finite threshold, rel_floor <= 0,
 * dilate or guided not 0 or 1, a non-zero reserved word (of the rule too), denoise.aov_spp > min_spp; mcpt_sequence_counts for a null
 * sequence or one created without a rule. */
typedef struct {
    mcpt_adaptive rule;  /* as mcpt_render_adaptive; the cap is each frame's params.spp */
    int32_t guided;      /* 0: the plain rule; 1: the threshold scaled by sqrt(history length) */
    int32_t reserved[7]; /* must be 0 */
} mcpt_sequence_adaptive; /* 64 bytes */
int mcpt_sequence_create_adaptive(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                  const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive, mcpt_sequence **out);
int mcpt_sequence_counts(mcpt_sequence *sequence, int32_t *spp_host, float *err_host, float *guide_host, mcpt_adaptive_info *info);

/* A sequence that reprojects what it sees through mirrors and glass.  A null or zeroed `motion`: mcpt_sequence_create_adaptive, exactly (the
 * same allocations, the same frame); with denoise.specular_depth 0 the switch changes nothing either.  With specular_motion 1 and
 * denoise.specular_depth D > 0, mcpt_sequence_frame changes in two places and nowhere else:
 *   step 4 is mcpt_render_motion_ex(camera, the previous frame's camera, params.seed, denoise.aov_spp, D);
 *   the history's depth plane and, with normal_test, its normal plane are written from channel 6 and channels 3..5 of the CHAIN AOVs of
 *   step 3 -- the depth a chain motion record's prev_depth measures -- and step 5 and the guide of an adaptive sequence read those; the
 *   extra first-hit AOV pass is neither run nor allocated.
 * Every output still equals what the separate calls give, bit for bit: mcpt_render_motion_ex, mcpt_temporal_accumulate[_ex],
 * mcpt_temporal_history_len and mcpt_denoise, with those planes as their prev_depth, normal and prev_normal arguments.
 * Allocated at create: the maps of the chains, 96 bytes per feature sample of a chunk of the motion pass, i.e. 96 * aov_spp bytes per
 * pixel (aov_spp 0 counts as 4) up to 96 MiB in all, in place of the 32 bytes per pixel of the first-hit AOVs.  A frame allocates nothing.
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_adaptive; specular_motion not 0 or 1, a non-zero reserved word. */
typedef struct {
    int32_t specular_motion; /* 0 | 1 */
    int32_t reserved[7];     /* must be 0 */
} mcpt_sequence_motion;      /* 32 bytes */
int mcpt_sequence_create_motion(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive,
                                const mcpt_sequence_motion *motion, mcpt_sequence **out);

/* A sequence whose history is weighted by sample counts.  A null or zeroed `weighted`: mcpt_sequence_create_motion, exactly (the same
 * allocations, the same frames).  With weighted 1 each history set gains a weight plane (4 bytes per pixel, 8 in all), and
 * mcpt_sequence_frame changes in these places and nowhere else:
 *   step 5 is mcpt_temporal_accumulate_weighted; its counts are the frame's count map (an adaptive sequence) or uniform_count =
 *   params.spp (a uniform one), its prev_weight the weight plane of the previous history set;
 *   with an adaptive rule and guided 1, step c is mcpt_temporal_history_weight and step d mcpt_render_adaptive_weighted with
 *   opts.temporal.max_history; the `guide` of mcpt_sequence_counts then reports the history weights H.
 * Every output still equals what the separate calls give, bit for bit.  A uniform sequence at a constant params.spp gives the outputs of
 * the unweighted sequence bit for bit, and weight = len * spp (mcpt_temporal_accumulate_weighted says why).  After a reset prev_len is 0,
 * so the weights restart at s.  The weights live in the alternating history sets: a failed frame leaves them as they were.
 * mcpt_sequence_weight copies the weights of the last successful frame to weight_host (W*H floats; all 0 before the first frame).
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_motion; weighted not 0 or 1, a non-zero reserved word;
 * mcpt_sequence_weight for a null pointer or a sequence created without weighted 1 (it keeps no weights). */
typedef struct {
    int32_t weighted;    /* 0 | 1 */
    int32_t reserved[7]; /* must be 0 */
} mcpt_sequence_weighted; /* 32 bytes */
int mcpt_sequence_create_weighted(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                  const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive,
                                  const mcpt_sequence_motion *motion, const mcpt_sequence_weighted *weighted, mcpt_sequence **out);
int mcpt_sequence_weight(mcpt_sequence *sequence, float *weight_host);

/* ---- Sequences at one sample per pixel: temporal luminance moments (the temporal half of SVGF, Schied et al. 2017).  The variance every
 * sequence above rests on is that of a frame's own samples, which needs two of them.  Here the history carries the running first and
 * second moment of each pixel's luminance instead, and the variance of the accumulated frame comes from the frames themselves.
 *
 * mcpt_temporal_accumulate_moments: the rule of mcpt_temporal_accumulate_ex without its three variance planes (none is read or written),
 * with two moments planes: prev_moments_host and out_moments_host, W*H*2 floats, {mu1, mu2} interleaved per pixel (0 everywhere for the
 * first frame).  Per pixel, in float, without contraction, in this order:
 *   l = (0.2126f * r + 0.7152f * g) + 0.0722f * b of the new colour;   m1 = l;   m2 = l * l;
 *   where the rule takes history (step 5), over exactly the taps, weights w and sum sw the colour used, in tap order and from 0:
 *       sm1 = sm1 + w * prev_moments[tap].mu1;   hm1 = sm1 / sw;   out_mu1 = hm1 + (m1 - hm1) * k     (likewise mu2)
 *     with the colour's own k = 1.f / N; an hm1 or hm2 that is not finite (a tap's stored moment was not) gives out_mu = (m1, m2);
 *   where it takes none (steps 1 and 4): out_mu = (m1, m2).
 * The colour clamp moves the colour history only, never the moments.  out_color, out_len AND out_flags ARE THOSE OF
 * mcpt_temporal_accumulate_ex ON THE SAME INPUTS, BIT FOR BIT.
 * MCPT_ERR_ARG, before any device call: every case mcpt_temporal_accumulate_ex refuses (its variance arrays apart); a null
 * prev_moments_host or out_moments_host.
 *
 * mcpt_moments_variance: the variance of the accumulated frame's luminance from those moments.  moments_host W*H*2 and len_host W*H as
 * mcpt_temporal_accumulate_moments wrote them, flags_host W*H bytes (nullable: no pixel counts as clamped), aov_host W*H*8 the AOVs the filter
 * will read; out_variance_host W*H.  Per pixel p, with N = len[p] and clamped = flags != null && (flags[p] & 2), in float:
 *   its own moments are not finite (its colour was not):  v = +inf, which mcpt_denoise passes through;
 *   temporal branch, N >= min_len and not clamped:
 *       q = mu2 - mu1*mu1;   q = q > 0 ? q : 0;   v = q / (N - 1.f)
 *     -- the unbiased per-frame variance q N / (N - 1) divided by the N frames of a running mean.  Beyond max_history the mean is
 *     exponential and its variance smaller, so this over-estimates: the filter smooths more, never less;
 *   spatial branch, everything else (a short history after a disocclusion or a reset, a clamped one): over the window dy = -radius..radius
 *     (outer), dx = -radius..radius, p itself included, a pixel q counts if it is in the image, has finite moments and passes a binary
 *     gate on the AOVs: both uncovered (coverage <= 0); or both covered with n_p.n_q > 0 (x + (y + z)) and
 *       |z_p - z_q| <= (sigma_z * |grad_p . (dx, dy)| + 1e-3f * max(z_p, z_q)) + 1e-6f,   grad_p the depth gradient of mcpt_denoise;
 *       cnt = cnt + 1.f;  s1 = s1 + mu1_q;  s2 = s2 + mu2_q;   a = s1 / cnt;  b = s2 / cnt;  q = b - a*a;  q = q > 0 ? q : 0;
 *       sig2 = q * (cnt / (cnt - 1.f));   cnt < 2: sig2 = mu2_p (a variance never exceeds the second moment);
 *       v = sig2 / (clamped ? 1.f : N).
 *     The spatial estimate takes undemodulated luminance, so texture contrast inside the window counts as noise: it over-smooths only.
 * opts.enabled is checked (0 | 1) and otherwise ignored here.
 * MCPT_ERR_ARG, before any device call: a null scene, moments_host, len_host, aov_host, opts or out_variance_host; width or height <= 0
 * or a frame too large; an option out of range or NaN; a non-zero reserved word. */
typedef struct {
    int32_t enabled;     /* 0 | 1 (mcpt_sequence_create_moments) */
    int32_t min_len;     /* the shortest history whose variance is temporal; 0 => 4; 2..4096 */
    int32_t radius;      /* of the spatial window; 0 => 3; 1..4 */
    float sigma_z;       /* of the window's depth gate; 0 => 1; > 0 and finite */
    int32_t reserved[4]; /* must be 0 */
} mcpt_moments_opts;     /* 32 bytes */
int mcpt_temporal_accumulate_moments(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *motion_host,
                                     const float *normal_host, const float *prev_color_host, const float *prev_depth_host,
                                     const float *prev_len_host, const float *prev_normal_host, const float *prev_moments_host,
                                     const mcpt_temporal_opts *opts, const mcpt_history_opts *history_opts, float *out_color_host,
                                     float *out_len_host, uint8_t *out_flags_host, float *out_moments_host);
int mcpt_moments_variance(mcpt_scene *scene, int32_t width, int32_t height, const float *moments_host, const float *len_host,
                          const uint8_t *flags_host /* nullable */, const float *aov_host, const mcpt_moments_opts *opts,
                          float *out_variance_host);

/* A sequence that takes its variance from temporal moments, and so runs at params.spp 1.  A null or zeroed `moments`:
 * mcpt_sequence_create_weighted, exactly (the same allocations, the same frames; such a sequence keeps refusing params.spp < 2).  With
 * enabled 1 each history set gains a moments plane (8 bytes per pixel, 16 in all), the 48 bytes per pixel of the render's moments are not
 * allocated, and mcpt_sequence_frame changes in these places and nowhere else:
 *   step 1 accepts params.spp >= 1 (denoise.aov_spp 0 => min(4, params.spp); aov_spp <= params.spp still holds);
 *   step 2 is the plain frame: fb is mcpt_render's frame bit for bit, and no moments of the render are summed;
 *   step 5 is mcpt_temporal_accumulate_moments between the alternating history sets;
 *   step 5b, right after it, is mcpt_moments_variance(the new set's moments and len, this frame's flags -- null for a sequence without
 *      history rejection --, the AOVs of step 3 -- the chain AOVs with specular_depth > 0 --; moments) into the variance plane that step 6
 *      and outputs.variance read.  ms_accumulate covers steps 5 and 5b.
 * Every output still equals what the separate calls give, bit for bit.  After a reset prev_len is 0, so the moments restart; they live in
 * the alternating history sets, so a failed frame leaves them as they were.  It combines with history rejection and with specular motion.
 * mcpt_sequence_moments copies the moments of the last successful frame to moments_host (W*H*2 floats; all 0 before the first frame).
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_weighted; enabled not 0 or 1, an option out of range or NaN, a non-zero
 * reserved word; enabled 1 with an adaptive rule (its counts need min_spp >= 2 and bring their own variance) or with weighted 1 (a
 * one-sample sequence has uniform counts, where weighting changes nothing); mcpt_sequence_moments for a null pointer or a sequence created
 * without moments. */
int mcpt_sequence_create_moments(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                 const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive,
                                 const mcpt_sequence_motion *motion, const mcpt_sequence_weighted *weighted, const mcpt_moments_opts *moments,
                                 mcpt_sequence **out);
int mcpt_sequence_moments(mcpt_sequence *sequence, float *moments_host);

/* ---- Pixel-centre feature rays.  Feature sample k above is the camera ray of render sample k: it carries the pixel jitter and the lens
 * sample, so a pixel's features change with the seed, and under depth of field one such ray lands anywhere inside the circle of
 * confusion.  With centre 1 the features of pixel m come from ONE deterministic ray instead, the centre ray of mcpt_centre_rays: through
 * the pixel centre and the centre of the lens.  It is the camera ray of Renderer.cpp:44-76 for the uniforms u = {0.5f, 0.5f, 0.f, 0.f}
 * in place of the Philox draw, every expression in its order, in float, without contraction:
 *   i = m % W, j = m / W;   x = (1 - 2 * (i + 0.5f) / (float) W) * aspect * scale;   y = (1 - 2 * (j + 0.5f) / (float) H) * scale;
 *   without depth of field  pos = eye,  dir = orient * normalized((x, y, 1));
 *   with depth of field     focal_point = (x, y, 1) * focal_distance;  r = aperture_radius * sqrtf(0.f);  sin = +0.f and cos = 1.f, the
 *                           bits the library's sincos gives at theta = 0;  dx = r * cos;  dy = r * sin;
 *                           pos = eye + orient * (dx, dy, 0);  dir = orient * normalized(focal_point - (dx, dy, 0))
 *   (normalized(v) = v / sqrtf(v.v) and the 3 x 3 products in the 3-term order a*x + (b*y + c*z), as for every camera ray).
 * So a finite aperture gives pos = eye + orient * (0, 0, 0) and the direction through the focal point: the pinhole ray up to rounding.
 * The ray is a function of the camera alone.  Everything behind it is unchanged: the closest-hit traversal, the first-hit records or the
 * chains of mcpt_render_aovs_ex / mcpt_render_motion_ex (whose branch rule, kr > 0.5, is deterministic already) and the folds, at one
 * sample per pixel.  A centre AOV or motion record therefore depends on scene, snapshot and cameras only, never on the seed: a static
 * pixel's record is bit-identical from frame to frame, and the motion of a moving surface is that of the point the pinhole sees.
 *
 * mcpt_render_aovs_features / mcpt_render_motion_features: a null or zeroed `features` makes the call mcpt_render_aovs_ex /
 * mcpt_render_motion_ex, exactly (the same kernels on the same keys).  With centre 1:
 *   aov_spp must be 0 or 1, and 0 means 1;   seed is ignored;   the key arrays of the pass are neither written nor read;
 *   the fold of one record: coverage and valid are exactly 0 or 1, the normal is the hit's unit normal (or 0), dx, dy, prev_depth those
 *   of the one sample.
 * MCPT_ERR_ARG, before any device call: every case of the _ex call; a centre that is not 0 or 1; a non-zero reserved word; aov_spp > 1
 * with centre 1.
 * Limits: inside a circle of confusion the guide's edges are sharper than the image's (the filter then stops at an edge the blur has
 * crossed); the halo of a moving blurred object takes the motion of the background its centre rays see, for which the colour clamp of
 * mcpt_history_opts is the remedy; pixels that see the sky have no depth to validate and still restart every frame. */
typedef struct {
    int32_t centre;      /* 0 | 1: features from the centre ray of each pixel */
    int32_t reserved[7]; /* must be 0 */
} mcpt_feature_opts;     /* 32 bytes */
int mcpt_render_aovs_features(mcpt_scene *scene, const mcpt_camera *camera, uint32_t seed, int32_t aov_spp, int32_t specular_depth,
                              const mcpt_feature_opts *features /* nullable */, float *aov_host);
int mcpt_render_motion_features(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_camera *prev_camera, uint32_t seed, int32_t aov_spp,
                                int32_t specular_depth, const mcpt_feature_opts *features /* nullable */, float *motion_host);

/* A sequence on centre features.  A null or zeroed `features`: mcpt_sequence_create_moments, exactly.  With centre 1 steps 3 and 4 of
 * mcpt_sequence_frame are mcpt_render_aovs_features and mcpt_render_motion_features with these options and aov_spp 1, and so are the
 * extra first-hit pass of specular_depth > 0 and the feature steps a and b of an adaptive sequence; nothing else changes, and every
 * output still equals what the separate calls give, bit for bit.  The chain maps of specular motion shrink to 96 bytes per pixel of a
 * chunk.  It combines with history rejection, specular motion, an adaptive rule, weighting and moments as those combine without it.
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_moments; a centre that is not 0 or 1; a non-zero reserved word;
 * centre 1 with opts.denoise.aov_spp > 1. */
int mcpt_sequence_create_features(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                  const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive,
                                  const mcpt_sequence_motion *motion, const mcpt_sequence_weighted *weighted, const mcpt_moments_opts *moments,
                                  const mcpt_feature_opts *features, mcpt_sequence **out);

/* ---- Filtered history (the feedback of SVGF, Schied et al. 2017).  Above, every frame's filter starts again from the raw running mean.
 * With feedback the records after a-trous iteration k become the colour history of the next frame, so that the spatial and the temporal
 * averaging compound.  Per pixel m, with r the record after iteration k (1 <= k <= the resolved iterations: the records iteration k + 1
 * reads), A_c = max(albedo_c, 1e-3) and la = lum(A), in float, without contraction (csrc/mcpt_denoise.h: dn::feedback_pixel):
 *   r usable (r.v >= 0):   feedback_color[3m + c] = r.e[c] * A_c   (the expression of step 4 of the filter);
 *                          feedback_variance[m]   = r.v * (la * la)  (the scaling of step 1 undone);
 *   otherwise:             colour and variance of the pixel pass through with their bits.
 *
 * mcpt_denoise_feedback: a null or zeroed `feedback` makes the call mcpt_denoise, exactly, and leaves the two feedback arrays untouched.
 * Otherwise out_host is mcpt_denoise's output bit for bit (the same kernels in the same order, one more behind iteration k, which only reads)
 * and feedback_color_host (W*H*3) and feedback_variance_host (W*H; nullable) hold the rule above at iteration `iteration`.
 * MCPT_ERR_ARG, before any device call: every case of mcpt_denoise; an iteration outside 0..8 or above the resolved iterations; a non-zero
 * reserved word; iteration > 0 with a null feedback_color_host. */
typedef struct { int32_t iteration; int32_t reserved[7]; } mcpt_feedback_opts;   /* 32 bytes; iteration 0 = off, else 1..8 */
int mcpt_denoise_feedback(mcpt_scene *scene, int32_t width, int32_t height, const float *color_host, const float *variance_host,
                          const float *aov_host, const mcpt_denoise_opts *opts, const mcpt_feedback_opts *feedback /* nullable */,
                          float *out_host, float *feedback_color_host, float *feedback_variance_host /* nullable */);

/* A sequence with a filtered history.  A null or zeroed `feedback`: mcpt_sequence_create_features, exactly (the same allocations, the same
 * frames).  With iteration k > 0 each history set gains a fed colour plane (12 bytes per pixel) and, unless the sequence keeps moments, a fed
 * variance plane (4): up to 32 bytes per pixel more, allocated at creation.  In mcpt_sequence_frame
 *   step 5 reads the previous set's fed colour as prev_color and its fed variance as prev_variance; depth, len, normals, flags and moments
 *      are read as before (the moments of a moments sequence stay those of the raw luminance);
 *   step 6 is mcpt_denoise_feedback(accumulated, the accumulated variance, the AOVs; opts.denoise; k), whose feedback arrays are the new
 *      set's fed planes.
 * outputs.accumulated stays the unfiltered blend of step 5 -- now of the new frame with a filtered history -- and outputs.variance and
 * outputs.denoised stay as defined.  Every output still equals the composition of the separate calls, bit for bit:
 * mcpt_temporal_accumulate_ex (or _moments, then mcpt_moments_variance) with the previous frame's feedback colour and variance as prev_color
 * and prev_variance, then mcpt_denoise_feedback.  The fed planes live in the alternating history sets, so a failed or refused frame leaves
 * them as they were; after mcpt_sequence_reset prev_len is 0 and they are not read.
 * mcpt_sequence_history copies the history the next frame will read: the fed planes of a feedback sequence, otherwise the colour and the
 * variance of the last successful frame's set; color_host W*H*3, variance_host W*H (nullable); all 0 before the first frame.
 * MCPT_ERR_ARG, before any device call: as mcpt_sequence_create_features; an iteration outside 0..8 or a non-zero reserved word; k > 0
 * with opts.filter 0, with k above the resolved iterations, with an adaptive rule or with weighted 1; mcpt_sequence_history for a null
 * sequence or colour pointer, and for a non-null variance_host on a moments sequence with feedback (it keeps no fed variance).
 * It combines with history rejection, specular motion, moments and centre features.
 * Limits: no adaptive rule and no weighting; mcpt_group_* has no sequence; the variance of a moments sequence describes the unfiltered
 * mean, so with feedback the filter over-smooths rather than under-smooths (as in SVGF); pixels that see the sky still restart every frame. */
int mcpt_sequence_create_feedback(mcpt_scene *scene, int32_t width, int32_t height, const mcpt_sequence_opts *opts,
                                  const mcpt_history_opts *history_opts, const mcpt_sequence_adaptive *adaptive,
                                  const mcpt_sequence_motion *motion, const mcpt_sequence_weighted *weighted, const mcpt_moments_opts *moments,
                                  const mcpt_feature_opts *features, const mcpt_feedback_opts *feedback, mcpt_sequence **out);
int mcpt_sequence_history(mcpt_sequence *sequence, float *color_host, float *variance_host /* nullable */);

/* Replaces Scene::intersect (Scene.hpp:128, Scene.cpp:19-21) for a list of rays (host pointers; n*3 floats each).
 * out_t: hit distance as the reference's double Intersection::distance (DBL_MAX on a miss);
 * out_prim: global primitive id (triangle index, or n_triangles + object index for a sphere; -1 on a miss). */
int mcpt_intersect(mcpt_scene *scene, int64_t n, const float *origins, const float *dirs, double *out_t,
                   int32_t *out_prim);

/* Replaces Scene::castRay(ray, 0, channel) (Scene.hpp:131, Scene.cpp:85-184) for a list of rays (host pointers).
 * The RNG of ray i is keyed by (params->seed, pixel[i], sample[i], channel[i]). */
int mcpt_cast_rays(mcpt_scene *scene, const mcpt_params *params, int64_t n, const float *origins, const float *dirs,
                   const uint32_t *pixel, const uint32_t *sample, const int32_t *channel, float *out);

/* Camera ray generation of Renderer.cpp:44-76 for (pixel m, sample k) pairs (host pointers); origins/dirs: n*3 floats. */
int mcpt_camera_rays(mcpt_scene *scene, const mcpt_camera *camera, uint32_t seed, int64_t n, const uint32_t *pixel,
                     const uint32_t *sample, float *origins, float *dirs);

/* The centre rays (mcpt_feature_opts above) of the n pixels pixel[0 .. n-1] (host pointers); origins/dirs: n*3 floats.  No seed and no
 * sample: the ray is a function of the camera.  MCPT_ERR_ARG for a null pointer with n > 0, n < 0 or above 2^31 - 1, width or height <= 0. */
int mcpt_centre_rays(mcpt_scene *scene, const mcpt_camera *camera, int64_t n, const uint32_t *pixel, float *origins, float *dirs);

/* ---- Ray queries on device memory: mcpt_intersect for rays that already sit in the memory of the scene's device, with the attributes
 * of the hit, and an any-hit (occlusion) query.  Rays are read from and results written to device memory, the work is enqueued on the
 * caller's stream and the calls return without synchronising the device: the caller's data must be ready in stream order, results are
 * ready in stream order.  Nothing is written beyond element n of any output.  Staging lives in buffers the scene owns, which only ever
 * grow: a call allocates only when it stages more rays than any call before it (mcpt_query_info::grew); rays are processed in chunks of
 * at most MCPT_QUERY_CHUNK rays (environment, read at scene creation; default 2^20, at least 64).
 *
 * mcpt_query_closest, tmax == NULL: t and prim of every ray are bit for bit what mcpt_intersect gives on the same scene for the same ray.
 * The occlusion rule: with t_i that distance and eps = (double)1e-4f (the render loop's EPSILON), ray i is occluded iff
 * t_i - (double)tmax[i] <= -eps, the occluder rule of the render loop's shadow rays with the light distance tmax.  So tmax = +inf asks
 * "is anything hit", and a NaN or a non-positive tmax is never occluded.
 * mcpt_query_closest with tmax: a ray reports its closest hit iff the rule holds for it, a miss otherwise (the finished closest hit is
 * filtered, so prim[i] >= 0 exactly where mcpt_query_occluded gives 1 for the same tmax).
 * mcpt_query_occluded: occluded[i] = 1 or 0 by the rule; the walk stops at the first primitive that proves occlusion.
 *
 * Both see the scene as it is now (after mcpt_scene_update / _deform / _set_visibility / _add_objects: as a freshly created scene of the
 * edited description; hidden objects are not hit).  The scene records one event on the caller's stream behind each query; every call
 * that swaps or frees geometry arrays or the staging buffers (the four above, mcpt_scene_set_materials when it rebuilds, and
 * mcpt_scene_destroy) waits for it on the host first, and a query on another stream waits for it on the device before it reuses the
 * staging buffers.  So an edit issued right after an enqueued query leaves that query's results correct.
 *
 * MCPT_ERR_ARG, before any device work: a null scene; n < 0 or n > 2^31 - 1; n > 0 with a null rays, origins or dirs; a null occluded or
 * tmax for mcpt_query_occluded; every hit pointer null; a pointer that hipPointerGetAttributes does not place on the scene's device.
 * n == 0 is a valid no-op.  A group's replicas are queried through mcpt_group_scene. */
typedef struct {            /* all pointers: memory of the scene's device, C-contiguous float32 */
    const float *origins;   /* n*3 */
    const float *dirs;      /* n*3, need not be normalised: t is in units of |d|, as in mcpt_intersect */
    const float *tmax;      /* n; closest: nullable (no limit); occluded: required */
} mcpt_ray_buffers;

typedef struct {            /* every member nullable; at least one non-null */
    double  *t;             /* n   the double mcpt_intersect returns, DBL_MAX on a miss */
    int32_t *prim;          /* n   global primitive id, -1 on a miss */
    int32_t *object;        /* n   index of the object in the scene's current object order (after mcpt_scene_add_objects: the extended order), -1 on a miss */
    float   *uv;            /* n*2 triangles: the barycentrics (u, v) of the test that recorded the hit, each rounded once to float; spheres and misses: 0, 0 */
    float   *normal;        /* n*3 the geometric normal of the scene's record (triangles), (p - c) normalised (spheres); misses: 0, 0, 0.  Never flipped towards the ray. */
    float   *point;         /* n*3 triangles: v0 + u e1 + v e2 on the live record (the rule of the motion pass); spheres: o + d (float)t; misses: 0, 0, 0 */
} mcpt_hit_buffers;

typedef struct {
    int32_t launches;       /* chunks the call was processed in */
    int32_t grew;           /* 1: the call had to allocate */
    int64_t staged_bytes;   /* device memory the scene holds for queries after the call */
    int32_t reserved[4];
} mcpt_query_info;

int mcpt_query_closest(mcpt_scene *scene, int64_t n, const mcpt_ray_buffers *rays, const mcpt_hit_buffers *hits, void *hip_stream,
                       mcpt_query_info *info /* nullable */);
int mcpt_query_occluded(mcpt_scene *scene, int64_t n, const mcpt_ray_buffers *rays, uint8_t *occluded /* n, device */, void *hip_stream,
                        mcpt_query_info *info /* nullable */);

/* ---- Radiance at sensors: the radiometric companion of the ray queries.  How much light arrives along a ray, or at a surface point, for
 * sensors that already sit in the memory of the scene's device: light probes, lightmap and irradiance baking, radiance caches,
 * path-traced targets for rays of a training loop.  A set of n sensors is rendered as a frame whose pixels are the sensors.
 *
 * Let ray(i, k) be the first ray of sensor i, sample k, and v(i, k, c) what mcpt_cast_rays returns on the same scene for that ray with
 * pixel = i, sample = params.sample_offset + k, channel = c and the same seed, rr_rate, n_dir_sample, enable_shadow and max_depth.  Then
 *   radiance[3i + c] = the float fold  acc = (accumulate ? radiance[3i + c] : 0); for k in 0 .. spp-1: acc += v(i, k, c) / spp_total,
 *                      spp_total = params.spp_total ? params.spp_total : params.spp   (the arithmetic of a pixel of mcpt_render), bit for bit;
 *   variance[3i + c] = max(s2/n - (s1/n)^2, 0) * n/(n-1) / n  with n = spp, s1 = sum v, s2 = sum v*v summed in double in sample order,
 *                      evaluated in double and rounded once to float: the variance of the channel's mean.
 * A non-null variance needs spp >= 2 and accumulate == spp_total == sample_offset == 0.  Progressive calls (sample_offset, spp_total,
 * accumulate) compose as they do for mcpt_render.
 *
 * Sensor kinds:
 *   MCPT_SENSOR_RAY         ray(i, k) = (origins[i], dirs[i]) for every k; the direction is used as given, exactly as mcpt_cast_rays uses
 *                           it.  No random numbers are spent on the ray.
 *   MCPT_SENSOR_HEMISPHERE  origins[i] is a surface point p, dirs[i] its unit normal n.  With u the four uniforms of the Philox block
 *                           (seed, i, sample_offset + k, stream 4) -- the channel paths use streams 0..2, the camera 3 --
 *                           r = sqrtf(u[0]), phi = 2 pi u[1], local = (r cos phi, r sin phi, sqrtf(1 - u[0])), the direction is
 *                           normalized(toWorld(local, n)) (Material.hpp:95-106) and the origin p + n * 1e-4f (Scene.cpp:114).  The
 *                           result is the cosine-weighted mean of the incoming radiance, E / pi: multiplied by an albedo it is the
 *                           Lambertian exitant radiance, what a lightmap stores.
 * mcpt_sensor_rays returns ray(sensor[j], sample[j]) for sensors given on the host (host pointers, like mcpt_camera_rays; `sample` is
 * absolute; origins and dirs have a row for every sensor the pairs name); for kind RAY these are the inputs of the named sensors.
 *
 * mcpt_query_radiance blocks like mcpt_render_device: the work is issued on hip_stream (the caller's data must be ready in stream order)
 * and the call returns when the outputs are written; sensors and outputs never leave the device.  The wavefront workspace and the
 * result buffers are the scene's own, sized as for a frame of n pixels; params.spp_per_pass and params.pool_paths are honoured.  stats
 * is filled as for a frame of n pixels (samples = n * spp); mcpt_scene_ray_counts and mcpt_scene_primary_conductor_counts describe the
 * call afterwards.  MCPT_ERR_OVERFLOW is returned as by mcpt_render, with the outputs written.  The call sees the scene as it is now.
 * Non-finite or all-zero inputs are not checked: such a sensor behaves as mcpt_cast_rays does for the same ray.  The reference's
 * per-level clamps bias the radiance of a sensor exactly as they bias a pixel.
 *
 * MCPT_ERR_ARG, before any device work: a null scene, params, sensors or out; n < 0 or n > (2^31 - 1) / 3; an unknown kind or a non-zero
 * reserved word; nranks > 1 or a non-zero rank; spp <= 0, n_dir_sample <= 0 or rr_rate not positive; the variance conditions above; with
 * n > 0 a null origins, dirs or radiance, or a pointer that hipPointerGetAttributes does not place on the scene's device.  n == 0 is a
 * valid no-op.  There is no mcpt_group_* form: mcpt_group_scene hands out the replicas, each of which can be asked. */
enum { MCPT_SENSOR_RAY = 0, MCPT_SENSOR_HEMISPHERE = 1 };
typedef struct {            /* device memory of the scene's device, float32, C-contiguous */
    const float *origins;   /* n*3  RAY: ray origin.        HEMISPHERE: surface point p */
    const float *dirs;      /* n*3  RAY: direction, used as given, exactly as mcpt_cast_rays uses it.  HEMISPHERE: unit normal */
    int32_t kind;           /* MCPT_SENSOR_* */
    int32_t reserved[3];    /* must be 0 */
} mcpt_sensor_buffers;      /* 32 bytes */
typedef struct {            /* device memory */
    float *radiance;        /* n*3, required */
    float *variance;        /* n*3, nullable: variance of each channel's mean */
} mcpt_sensor_outputs;      /* 16 bytes */
int mcpt_query_radiance(mcpt_scene *scene, const mcpt_params *params, int64_t n, const mcpt_sensor_buffers *sensors,
                        const mcpt_sensor_outputs *out, void *hip_stream, mcpt_stats *stats /* nullable */);
int mcpt_sensor_rays(mcpt_scene *scene, int32_t kind, uint32_t seed, int64_t n, const float *origins, const float *dirs,
                     const uint32_t *sensor, const uint32_t *sample, float *origins_out, float *dirs_out);

/* Tone map of Renderer.cpp:95-103 on the GPU: rgba[4i + c] = (unsigned char) clamp(0, 255, 255 * pow(fb[3i + c], 0.45f)), alpha 255,
 * NaN -> 255 as the reference's std::min/std::max clamp gives.  std::pow is the library's own plain-IEEE pow (csrc/mcpt_fmath.h), within
 * an ulp of any libm's.  Optional: the float frame of mcpt_render is the boundary's product; callers may keep their own tone map. */
int mcpt_tonemap(mcpt_scene *scene, const float *fb_host, int64_t n_pixels, uint8_t *rgba_host);
int mcpt_tonemap_device(mcpt_scene *scene, const float *fb_device, int64_t n_pixels, uint8_t *rgba_device, void *hip_stream);

/* ---- Multi-GPU inside the boundary.  The caller stays single-threaded like the reference's main() (Renderer::Render blocks,
 * main.cpp:333): a group holds one replica of the scene per device; mcpt_group_render partitions the frame into interleaved
 * tiles over the devices (tile_size of `params`, default 32; its rank/nranks fields are ignored), drives every device from its
 * own host thread, sums the per-device frames into the first device's with one RCCL ncclReduce over xGMI and returns the
 * merged frame in fb_host.  The result is bit-identical to mcpt_render on one GPU (disjoint pixels, same Philox keys).
 * `devices`: distinct HIP device indices; as a rehearsal on a one-GPU box every entry may name the SAME device (the merge is
 * then a kernel on that device; RCCL is neither loaded nor needed).  Errors of these three calls: mcpt_group_last_error(). */
typedef struct mcpt_group mcpt_group;
int mcpt_group_create(const mcpt_scene_desc *desc, int n_devices, const int *devices, mcpt_group **out);
int mcpt_group_render(mcpt_group *group, const mcpt_camera *camera, const mcpt_params *params, float *fb_host, mcpt_stats *stats);
int mcpt_group_size(const mcpt_group *group);
/* What mcpt_group_create spent: the scene is flattened and its tree built once (build_ms) while every device is brought up on a helper
 * thread (init_ms_max), then one thread per device copies it (upload_ms_max); setup_ms is the wall clock of the whole call. */
typedef struct {
    int32_t n_devices;
    int32_t uses_rccl; /* 1: distinct devices, the frames are merged by one ncclReduce; 0: every entry names one device (rehearsal) */
    double build_ms, upload_ms_max, init_ms_max, setup_ms;
} mcpt_group_info;
int mcpt_group_get_info(const mcpt_group *group, mcpt_group_info *info);
/* The replica on the index-th device of the group (borrowed: it lives as long as the group), for calls that take a scene, e.g.
 * mcpt_tonemap after mcpt_group_render.  NULL when out of range. */
mcpt_scene *mcpt_group_scene(mcpt_group *group, int index);
/* mcpt_scene_update on every replica (one host thread per replica), with the same checks before any device call.  If a replica fails,
 * the replicas that had succeeded are given their previous transforms back, so that the group stays one scene. */
int mcpt_group_update(mcpt_group *group, int32_t n, const mcpt_object_transform *moves);
/* mcpt_scene_set_materials / mcpt_scene_set_environment on every replica, with the same checks before any device call.  If a replica
 * fails, the replicas that had changed get their previous materials (environment) back: the group stays one scene. */
int mcpt_group_set_materials(mcpt_group *group, int32_t n_edits, const mcpt_material_edit *edits, int32_t n_assign,
                             const mcpt_object_material *assign);
int mcpt_group_set_environment(mcpt_group *group, const float background[3], int32_t env_w, int32_t env_h, const float *env_pixels);
/* mcpt_scene_deform on every replica, host pointers only: an item with on_device 1 is refused with MCPT_ERR_ARG, since one pointer
 * cannot be valid on several devices.  If a replica fails, the replicas that had succeeded get their previous positions back. */
int mcpt_group_deform(mcpt_group *group, int32_t n, const mcpt_object_vertices *items);
/* mcpt_scene_set_visibility on every replica, with the same checks before any device call.  If a replica fails, the replicas that had
 * succeeded get their previous mask back. */
int mcpt_group_set_visibility(mcpt_group *group, int32_t n, const mcpt_object_visibility *items);
/* mcpt_scene_add_objects on every replica, with the same checks once before any device call.  Every replica keeps its previous arrays
 * aside until all have succeeded; if one fails, the replicas that had grown get them back, counts and snapshot included. */
int mcpt_group_add_objects(mcpt_group *group, const mcpt_scene_addition *add, int32_t *first_object /* nullable */);
void mcpt_group_destroy(mcpt_group *group);
const char *mcpt_group_last_error(void);

/* Scene statistics for reporting (BVH nodes, tree height, bytes resident in HBM). */
typedef struct {
    int32_t n_nodes, bvh_height, n_lights, n_prims;
    uint64_t scene_bytes;
    double build_ms;  /* flattening + BVH build (the data producer of BVHAccel::recursiveBuild, BVH.cpp:27-93) */
    double upload_ms; /* host -> HBM copies */
    int32_t builder;  /* 0 host binned SAH, 1 host reference topology (median split), 2 GPU LBVH, 3 GPU PLOC */
    int32_t quantised;/* 1: 32-byte nodes with 16-bit boxes are traversed */
    int32_t n_instances; /* objects whose traversal nodes are shared with a prototype (0: plain tree) */
    int32_t lds_resident; /* 1: the scene is small enough for the kernels that copy nodes, triangles, spheres and light tables into LDS */
    double init_ms;   /* first use of the device by this process (context creation, load of the library's code objects), run on a helper
                         thread beside the host build; ~0 for every later scene.  Not part of build_ms / upload_ms */
} mcpt_scene_info;
int mcpt_scene_get_info(const mcpt_scene *scene, mcpt_scene_info *info);

/* The continuation rays (every closest-hit ray beyond the primary rays) of the scene's last frame-level render call or mcpt_cast_rays
 * call: `traced` walked the tree; `shared` are records that continued on the ray of a sibling channel path instead (the channel paths
 * of a sample leave a smooth-conductor vertex in one direction; MCPT_SHARE_RAYS=0 switches the sharing off).  traced + shared is what
 * mcpt_stats::closest_rays counts beyond the primary rays, so that field and ref_scene_rays do not depend on the sharing; how the sum
 * splits depends on the schedule (pool size, pass size, ranks).  Zero before the first call. */
int mcpt_scene_ray_counts(const mcpt_scene *scene, uint64_t *traced, uint64_t *shared);

/* First hits on smooth conductors that the primary-ray kernel finished itself in the scene's last frame-level render call (DESIGN.md
 * section 6; MCPT_PRIMARY_CONDUCTOR=0 switches it off): `samples` took that path -- their three channel paths were finished in the
 * kernel or handed on as ordinary records --, and `rays` of the `traced` count of mcpt_scene_ray_counts are reflected rays that kernel
 * walked itself, one per sample with a surviving channel, so traced - rays is what the closest-hit queue kernel walked.  (With
 * MCPT_SHARE_RAYS=0 `rays` counts one per surviving channel, as if each had stored its own.)  Zero before the first call. */
int mcpt_scene_primary_conductor_counts(const mcpt_scene *scene, uint64_t *samples, uint64_t *rays);

/* Host-only diagnostic (no GPU needed): builds the traversal tree of `desc` exactly as mcpt_scene_create does and copies it
 * out, so that the builder (the data producer of BVHAccel::recursiveBuild, BVH.cpp:27-93) can be checked on any machine.
 * Call with boxes == NULL to get the counts, then with arrays of n_nodes entries:
 *   boxes[n][12]    float  {lmin.xyz, lmax.xyz, rmin.xyz, rmax.xyz} of the two children
 *   children[n][2]  int32  child >= 0: inner node index; < 0: leaf, primitive id = ~child
 *   qboxes[n][12]   uint16 the same boxes on the 16-bit grid (only written when info->quantised)
 * Primitive ids: triangle index, or n_triangles + object index for a sphere.
 * With instancing, a leaf index (~child) >= n_leaf_prims is instance k = index - n_leaf_prims: the subtree at inst_root_first[k][0],
 * whose boxes are in the prototype's position (this object's position = prototype + inst_shift[k]) and whose leaves hold LOCAL
 * triangle indices (global id = inst_root_first[k][1] + local).  inst_* may be NULL. */
typedef struct {
    int32_t n_nodes, root, stack_entries, quantised;
    float root_min[3], root_max[3];
    float q_origin[3], q_cell[3]; /* grid coordinate q <-> q_origin + q * q_cell */
    int32_t n_instances, n_leaf_prims;
} mcpt_bvh_info;
int mcpt_bvh_dump(const mcpt_scene_desc *desc, mcpt_bvh_info *info, float *boxes, int32_t *children, uint16_t *qboxes,
                  float *inst_shift, int32_t *inst_root_first);
/* The same arrays downloaded from a live scene (whatever built its tree, the GPU builder included). */
int mcpt_scene_dump_bvh(mcpt_scene *scene, mcpt_bvh_info *info, float *boxes, int32_t *children, uint16_t *qboxes,
                        float *inst_shift, int32_t *inst_root_first);

/* Diagnostic: evaluates the path's transcendental functions (csrc/mcpt_fmath.h: the library's own plain-IEEE sin / cos /
 * atan2 / acos, used where the reference calls libm at Material.hpp:117-118, Renderer.cpp:59-60, Sphere.hpp:66-67,
 * Scene.hpp:66-67) ON THE DEVICE for n host floats, so that tests can check that kernels and a CPU build of the same
 * header agree bit for bit.  kind: 0 sin(x), 1 cos(x), 2 atan2(x, y), 3 acos(x), 4 pow(x, y), 5 tone-map byte of x (as a float);
 * y may be NULL unless kind is 2 or 4. */
int mcpt_debug_fmath(mcpt_scene *scene, int kind, int64_t n, const float *x, const float *y, float *out);

/* Diagnostic: evaluates the device's Material functions (csrc/mcpt_device.h, following Material.hpp:26-151,178-408) for n rows, so
 * that tests can compare them one by one -- not only through whole paths -- with the CPU restatement.  in: 13 floats per row
 * {a.xyz, b.xyz, c.xyz, uv.xy, u1, u2}; sel: 3 ints per row {material index, channel 0..2, is_reflect}; out: 4 floats per row.
 * kind 0 Material::eval(wi = a, wo = b, N = c, uv), 1 Material::pdf(a, b, c), 2 fresnel(I = a, N = b), 3 sample(N = a; u1, u2) -> xyz,
 * 4 refract(I = a, N = b) -> xyz, 5 the fused eval + pdf of the shading kernel -> {eval, pdf}, 6 reflect(I = a, N = b) -> xyz. */
int mcpt_debug_material(mcpt_scene *scene, int kind, int64_t n, const float *in, const int32_t *sel, float *out);

/* Diagnostic: the device's Scene::sampleLight (Scene.cpp:23-37 with MeshTriangle::Sample, BVHAccel::getSample, Triangle::Sample; kind 0:
 * in = 4 uniforms per row {light choice, triangle pick, x, y}, out = 10 floats per row {point, normal, emission, pdf}) and
 * Scene::sampleEnv (Scene.hpp:60-99; kind 1: in = a direction per row, out = rgb) on arrays. */
int mcpt_debug_scene(mcpt_scene *scene, int kind, int64_t n, const float *in, float *out);

/* Diagnostic: the shadow-visibility query of the render loop (k_trace_shadow and, for trees that use the retry flavour of the
 * traversal stack, k_retrace_shadow: the product's own launch, unchanged) for n rays of the caller's, so that tests can compare it
 * ray by ray with the rule of Scene.cpp:74-75: a light sample is visible iff the CLOSEST hit of the ray lies within EPSILON (1e-4)
 * of the light distance.  origins, dirs: n x 3 floats; dist: n floats, finite and > 0; visible: n bytes, 1 or 0.
 * The call fills a shadow queue of its own exactly as the direct-lighting kernel leaves it: ray i goes to shard shard[i] (0..31;
 * shard == NULL: shard (i / 64) % 32, where a wave of that kernel would put it), entries with found[i] == 1 from the front of the
 * shard's region, the others from its back; the queue's capacity is the smallest whose region holds the fullest shard.  list (0 or
 * 1) selects which of the two sets of per-shard counters carries the counts, as the path list a launch belongs to does.
 * found[i] == 1 is the caller's ASSERTION that some primitive is hit within EPSILON of dist[i] -- what the direct-lighting kernel
 * has established by testing the sampled light primitive when it sets the flag.  The query then skips its window search and only
 * looks for an occluder.  With a false assertion the call returns what the render loop would compute from such an entry; nothing
 * is promised about that value.  found[i] == 0 is always truthful: the full query runs.
 * Origins are expected at scene scale, like every origin of the render loop (a point on a surface).
 * Memory: the queue holds 32 regions of the fullest shard's size (rounded up to 64 entries), 32 bytes per entry, on the host and on
 * the device: 8 MiB per 2^18 rays with the default placement, 2 x 2 GiB for 2^22 rays placed in ONE shard (MCPT_ERR_OOM if that fails).
 * MCPT_ERR_ARG, before any device call: a null scene; list outside 0..1; n < 0 or n > 2^22; n > 0 with a null array other than
 * shard; a shard index outside 0..31; found[i] > 1; a dist[i] that is not finite or not > 0.  n == 0 is a valid no-op. */
int mcpt_debug_shadow(mcpt_scene *scene, int32_t list, int64_t n, const float *origins, const float *dirs, const float *dist,
                      const uint8_t *found, const int32_t *shard /* nullable */, uint8_t *visible);

/* ---- Diagnostics of the sky cull (csrc/mcpt_cull.hip): the conservative per-pixel classification in front of every render.
 *
 * mcpt_cull_bound: host only, no GPU needed.  The geometric bound the classifier would use for `camera` over a scene whose root box is
 * [root_min, root_max]: every camera ray of a pixel stays within rho of the pixel's central ray (pixel centre, lens centre) at equal
 * parameter, as long as it is inside the root box.  It is the very function the render path calls.
 *   classified  0: the camera is outside what the bound covers (a matrix that is not orthonormal, an aperture or pixel footprint too
 *               large for the focal distance, a non-finite value); nothing is culled and rho is 0
 *   rho         the widening of every box as the kernel gets it: 1.05 x the bound + a rounding allowance
 *   scale, aspect, focal, lens   what the classifier reads of the camera: scale = tan(fov/2) and aspect = W/H exactly as the camera rays
 *               use them; focal distance (1 without depth of field); aperture radius (0 without)
 *   h, s_far, reach, fmin        the terms of the bound, in double (0 where the refusal came before they were formed)
 * MCPT_ERR_ARG for a null pointer or a width or height <= 0. */
typedef struct {
    int32_t classified;
    float rho, scale, aspect, focal, lens;
    double h, s_far, reach, fmin;
} mcpt_cull_info; /* 56 bytes */
int mcpt_cull_bound(const mcpt_camera *camera, const float root_min[3], const float root_max[3], mcpt_cull_info *info);

/* The classifier itself (the product's own launch, unchanged) for all W*H pixels of `camera` in pixel order m = j*W + i, as the kernel
 * wrote it, before the pixels are partitioned:
 *   may_hit[m]      0: no camera ray of the pixel can hit anything; 1: one might
 *   cand[4m..4m+3]  the primitives every ray of the pixel can hit, as primitive ids (mcpt_intersect) in the order the walk found them,
 *                   unused slots -1; or {-2, -1, -1, -1}: more than four, or an instance: the pixel's rays walk the tree
 * With info->classified == 0 every pixel reports may_hit 1 and "walk the tree".  info (nullable) is the bound as the kernel got it:
 * mcpt_cull_bound on the scene's root box.  The call classifies whatever MCPT_SKY_CULL says and for environment-map scenes too: it is
 * the classifier, not the decision to use it.  MCPT_ERR_ARG, before any device call: a null pointer other than info, a width or
 * height <= 0, more than 2^26 pixels. */
int mcpt_debug_classify(mcpt_scene *scene, const mcpt_camera *camera, uint8_t *may_hit /* W*H */, int32_t *cand /* W*H*4 */,
                        mcpt_cull_info *info /* nullable */);

/* Diagnostic: counters of the checking build (libmcpt_hip_check.so, compiled with -DMCPT_CHECK_DIRECT_SKIP; the traversal
 * entries are filled only by a -DMCPT_TRAVERSAL_STATS build); all zero in the product build.
 *   out[0..5]   closest-hit rays: rays, node visits, primitive tests, hits, 64 x wave iterations, -
 *   out[8..13]  shadow rays: rays, node visits, primitive tests, occluded, 64 x wave iterations, found in the window
 *   out[10..13] (checking build) the counts of out[14] / out[15] for the vertices the total-internal-reflection rule claims (10, 11)
 *               and for those the half-space rule claims (12, 13)
 *   out[14]     light samples evaluated at vertices the product would have skipped as "provably zero" (direct_is_zero)
 *   out[15]     how many of those had a non-zero contribution (must be 0) */
int mcpt_debug_counters(mcpt_scene *scene, uint64_t out[16]);

/* ---- Lightmaps: from an object's UV layout to texel sensors, and from their radiance back to an image (csrc/mcpt_lightmap.h states the
 * rule once, for the host and the device; csrc/mcpt_lightmap.hip holds the kernels).
 *
 * Coverage.  Texel (x, y) of a width x height map has its centre at px = ((double)x + 0.5) / width, py = ((double)y + 0.5) / height.  A
 * triangle of the object with texture coordinates a = t0, b = t1, c = t2 (widened to double; never wrapped) covers it iff, with
 *   area2 = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax)                      zero or not finite: the triangle covers nothing
 *   w1 = ((px-ax)*(cy-ay) - (py-ay)*(cx-ax)) / area2,  w2 = ((bx-ax)*(py-ay) - (by-ay)*(px-ax)) / area2,  w0 = 1 - w1 - w2
 * all of w0, w1, w2 are >= 0 (a NaN fails).  Among the object's triangles that cover a texel the lowest global primitive id owns it;
 * the chart's winding does not matter.
 * Sensor.  bary = {(float)w1, (float)w2} = (u, v); origin = v0 + (e1*u + e2*v) per component in float on the LIVE triangle record (the
 * `point` of mcpt_query_closest); normal = the live record's normal, negated with flip_normals.  Together they are a sensor of kind
 * MCPT_SENSOR_HEMISPHERE, which applies its own offset along the normal.
 * Order.  Covered texels are listed in ascending texel index y*width + x; entry i is sensor i (Philox key (seed, i)).
 * Scatter and dilation.  image[texel[i]] = values[i], every other texel 0; coverage 1 where scattered.  Then `dilate` rounds: every texel
 * whose coverage is still 0 and that has n >= 1 of its 8 neighbours with coverage != 0 AT THE START OF THE ROUND takes, per channel, the
 * float sum of those neighbours (added to 0.f in the order (-1,-1) (0,-1) (1,-1) (-1,0) (1,0) (-1,1) (0,1) (1,1)) divided by (float)n,
 * and coverage 2.  A texel index listed twice gives one of its values; an index outside the map is ignored.
 *
 * MCPT_ERR_ARG, before any device work: a null scene, desc or required pointer; a non-zero reserved word; an object out of range or a
 * sphere; an instanced scene; width or height < 1 or width*height > (2^31 - 1) / 3; dilate < 0; n outside 0 .. width*height; a pointer
 * that is not memory of the scene's device.  An object without a covered texel: MCPT_OK, n_out = 0, a zero image.  A hidden object may be
 * asked: its records exist, and the light it receives is that of the scene without it. */
typedef struct {
    int32_t object, width, height, flip_normals;
    int32_t reserved[4]; /* must be 0 */
} mcpt_lightmap_desc; /* 32 bytes */
typedef struct { /* device memory, capacity width*height rows each; every member nullable except texel */
    int32_t *texel;
    int32_t *prim;  /* global primitive id of the owner */
    float *bary;    /* *2 */
    float *origins; /* *3 */
    float *normals; /* *3 */
} mcpt_lightmap_texels_out;
typedef struct {
    int64_t n_texels;   /* covered texels = sensors */
    int64_t items;      /* (triangle, 8x8 tile) pairs the rasteriser tested, one wave each */
    int32_t grew;       /* 1: a scene-owned buffer was allocated or enlarged in this call; 0 in the steady state */
    int32_t reserved0;
    double ms_texels, ms_radiance, ms_scatter; /* host wall clock of the three legs */
    int32_t reserved[4];
} mcpt_lightmap_info; /* 64 bytes */
/* Emits the object's texel sensors from the scene as it is now (after every update, deformation, addition) on hip_stream.  Blocks until
 * *n_out is known; the rows of prim, bary, origins, normals are then ready in stream order.  All staging is scene-owned and only grows. */
int mcpt_lightmap_texels(mcpt_scene *scene, const mcpt_lightmap_desc *desc, const mcpt_lightmap_texels_out *out, int64_t *n_out, void *hip_stream);
/* image (width*height*3 floats) and coverage (width*height bytes, nullable) from n values at the listed texels; enqueued on hip_stream
 * without a host synchronisation.  All pointers are device memory. */
int mcpt_lightmap_scatter(mcpt_scene *scene, const mcpt_lightmap_desc *desc, int64_t n, const int32_t *texel, const float *values /* n*3 */,
                          int32_t dilate, float *image /* W*H*3 */, uint8_t *coverage /* W*H, nullable */, void *hip_stream);
/* mcpt_lightmap_texels -> mcpt_query_radiance (kind hemisphere, on scene-owned sensor buffers) -> mcpt_lightmap_scatter: the map of
 * E / pi.  variance (nullable, needs spp >= 2): the variance of each texel's mean, scattered without dilation.  Blocks like
 * mcpt_render_device.  Also MCPT_ERR_ARG: nranks > 1 or rank != 0; non-positive spp, n_dir_sample or rr_rate; non-zero sample_offset,
 * spp_total or accumulate (progressive bakes are composed from the three pieces). */
int mcpt_bake_lightmap(mcpt_scene *scene, const mcpt_lightmap_desc *desc, const mcpt_params *params, int32_t dilate, float *image,
                       uint8_t *coverage /* nullable */, float *variance /* W*H*3, nullable */, void *hip_stream,
                       mcpt_lightmap_info *info /* nullable */, mcpt_stats *stats /* nullable */);
/* Host only, no GPU needed: the same header compiled for the CPU, on a description (as mcpt_compact_scene and mcpt_cull_bound are).  The
 * records are built by the routine scene construction uses, so a fresh scene of `desc` gives the same bits.  Arrays of width*height rows;
 * every array nullable (all null: only the count). */
int mcpt_lightmap_texels_host(const mcpt_scene_desc *desc, const mcpt_lightmap_desc *lightmap, int32_t *texel, int32_t *prim, float *bary,
                              float *origins, float *normals, int64_t *n_out);
int mcpt_lightmap_dilate_host(int32_t width, int32_t height, int64_t n, const int32_t *texel, const float *values, int32_t dilate,
                              float *image, uint8_t *coverage /* nullable */);

/* ---- Light probes: the incoming radiance over the whole sphere at points in free space, projected onto the nine real spherical
 * harmonics of order <= 2, and the irradiance of any normal from those 27 floats (csrc/mcpt_sh.h states the rule once, for the host and
 * the device; csrc/mcpt_probes.hip holds the kernels).  A regular grid of probes blended trilinearly is the irradiance volume.
 *
 * Basis, for a unit d = (x, y, z), in float with a*b*c = (a*b)*c:  Y0 = 0.28209479f, Y1 = 0.48860251f y, Y2 = 0.48860251f z,
 * Y3 = 0.48860251f x, Y4 = 1.0925484f x y, Y5 = 1.0925484f y z, Y6 = 0.31539157f (3 z z - 1), Y7 = 1.0925484f x z,
 * Y8 = 0.54627422f (x x - y y): the float roundings of sqrt(1/4pi), sqrt(3/4pi), sqrt(15/4pi), sqrt(5/16pi), sqrt(15/16pi).
 * First ray of (probe i, sample k): with u the uniforms of the Philox block (seed, i, sample_offset + k, stream 4), z = 1 - 2 u[0],
 * r = sqrtf(fmaxf(0, 1 - z z)), phi = 2 pi u[1], direction d(i, k) = normalized((r cos phi, r sin phi, z)), origin origins[i] itself (no
 * offset: a probe sits in free space).  mcpt_probe_rays returns these rays for probes given on the host, like mcpt_sensor_rays.
 * Projection, with v(i, k, c) as for mcpt_query_radiance and spp_total likewise:
 *   sh[27i + 3j + c]:  acc = accumulate ? sh[27i + 3j + c] : 0;  for k in 0 .. spp-1:  acc += (v(i,k,c) * (kFourPi * Y_j(d(i,k)))) / spp_total
 * in float, kFourPi = (float)(4 pi), the reciprocal of the uniform pdf.  radiance (nullable) is the plain fold of mcpt_query_radiance
 * over the same samples, the mean radiance over the sphere; variance (nullable) its variance under the same conditions.
 * Irradiance: mcpt_sh_irradiance_host gives E / pi for a unit normal n, out[c] = sum over j in index order, from 0, of
 * (A(j) * L[3j + c]) * Y_j(n), A = 1, 2/3 (j = 1..3), 1/4 (j = 4..8): the clamped-cosine convolution over pi.  It is NOT clamped at 0:
 * the truncated series rings and can go slightly negative.
 * Grid: probe (ix, iy, iz) sits at origin + (float)i * spacing per axis, index (iz * ny + iy) * nx + ix.  Lookup of a point p, per axis:
 * g = (p - origin) / spacing clamped to [0, dim - 1], i0 = min((int)floorf(g), dim - 2), t = g - i0; dim == 1: i0 = 0, t = 0 and the
 * missing neighbour is the probe itself.  Each of the 27 coefficients is blended over the eight corners, b = 0; b += w * L_corner in the
 * order (dz, dy, dx) = 000, 001, 010, .. 111, w = (wz * wy) * wx with w_axis = 1 - t or t; then the irradiance sum above.  No visibility
 * test: a probe inside an object reports what mcpt_cast_rays gives there.
 *
 * mcpt_query_probes blocks like mcpt_query_radiance, makes the same refusals before any device work, and also refuses n > (2^31 - 1) / 27;
 * n == 0, MCPT_ERR_OVERFLOW, stats and the ray counts follow the same rules; it sees the live scene as it is now.  mcpt_probe_shade is
 * enqueued on hip_stream without a synchronisation or an allocation.  mcpt_bake_probe_grid writes the grid's points into a scene-owned
 * buffer that only grows and runs mcpt_query_probes on it.  MCPT_ERR_ARG for a grid: a dims member < 1, more than (2^31 - 1) / 27
 * probes, a spacing that is not positive and finite, a non-zero reserved word.  No mcpt_group_* form (mcpt_group_scene). */
typedef struct {
    float origin[3], spacing[3];
    int32_t dims[3];     /* nx, ny, nz */
    int32_t reserved[3]; /* must be 0 */
} mcpt_probe_grid; /* 48 bytes */
typedef struct {        /* device memory */
    float *sh;          /* n*27, required */
    float *radiance;    /* n*3, nullable */
    float *variance;    /* n*3, nullable */
    void *reserved;     /* must be null */
} mcpt_probe_outputs;  /* 32 bytes */
int mcpt_query_probes(mcpt_scene *scene, const mcpt_params *params, int64_t n, const float *origins /* n*3, device */,
                      const mcpt_probe_outputs *out, void *hip_stream, mcpt_stats *stats /* nullable */);
int mcpt_probe_rays(mcpt_scene *scene, uint32_t seed, int64_t n, const float *origins, const uint32_t *sensor, const uint32_t *sample,
                    float *origins_out, float *dirs_out);
int mcpt_probe_shade(mcpt_scene *scene, const mcpt_probe_grid *grid, const float *sh /* probes*27, device */, int64_t n,
                     const float *points /* n*3, device */, const float *normals /* n*3, device */, float *out /* n*3, device */, void *hip_stream);
int mcpt_bake_probe_grid(mcpt_scene *scene, const mcpt_probe_grid *grid, const mcpt_params *params, float *sh /* probes*27, device */,
                         void *hip_stream, mcpt_stats *stats /* nullable */);
/* The floats the scene-owned probe buffers hold and how often one of them was (re)allocated: 0 more in the steady state. */
int mcpt_scene_probe_buffers(const mcpt_scene *scene, int64_t *floats, int64_t *allocations);
/* Host only, no GPU needed: csrc/mcpt_sh.h compiled for the CPU. */
int mcpt_sh_basis_host(int64_t n, const float *dirs /* n*3 */, float *basis /* n*9 */);
int mcpt_sh_irradiance_host(int64_t n, const float *sh /* n*27 */, const float *normals /* n*3 */, float *out /* n*3 */);
int mcpt_probe_grid_points_host(const mcpt_probe_grid *grid, float *points /* probes*3 */);
int mcpt_probe_shade_host(const mcpt_probe_grid *grid, const float *sh, int64_t n, const float *points, const float *normals, float *out);

/* ---- Probe visibility: a small octahedral map of distance moments per probe, a Chebyshev visibility weight at lookup and a back-face
 * count that retires buried probes, so that the irradiance volume above works next to walls and around objects (csrc/mcpt_probe_depth.h
 * states the rule once, for the host and the device; csrc/mcpt_probes.hip holds the kernels).  Float32 in the written order, no FMA;
 * only + - * /, sqrtf, fabsf, fminf, fmaxf, floorf.  dot(a, b) = a.x b.x + (a.y b.y + a.z b.z); sgn(v) = v >= 0 ? 1 : -1.
 *
 * Depth map: MCPT_PROBE_DEPTH_RES x MCPT_PROBE_DEPTH_RES = 8 x 8 texels per probe, texel j = 8 ty + tx.
 * Texel direction c_j: ox = ((float)tx + 0.5f) * 0.25f - 1.0f, oy likewise from ty; az = (1 - |ox|) - |oy|; if az < 0:
 * (x, y) = ((1 - |oy|) sgn(ox), (1 - |ox|) sgn(oy)), else (x, y) = (ox, oy); c = (x, y, az), each divided by sqrtf((x x + y y) + az az).
 * Texel of a vector v (nearest texel; v need not be unit): s = (|vx| + |vy|) + |vz|; if s is zero or not finite (not s > 0, or
 * s > FLT_MAX, or NaN) the texel is 0; else px = vx / s, py = vy / s; if vz < 0: (px, py) = ((1 - |py|) sgn(px), (1 - |px|) sgn(py))
 * from the old values; tx = clamp((int)floorf((px + 1) * 4), 0, 7), ty likewise from py.
 * Sample: d(i, k) is the direction mcpt_probe_rays gives for (seed, probe i, absolute sample sample_offset + k), t(i, k) the double
 * mcpt_intersect gives for that ray from origins[i], ng the normal mcpt_query_closest reports for the hit;
 * r = hit ? fminf((float)t, max_distance) : max_distance; the sample is back-facing iff it is a hit and dot(ng, d) > 0.
 * Fold, per (probe i, texel j): w = fmaxf(dot(c_j, d), 0), then w = w * w five times (cos^32).  moments[(64 i + j) * 3 + 0..2] =
 * (W, S1, S2): acc = accumulate ? existing : 0; for k in sample order: W = W + w; S1 = S1 + w * r; S2 = S2 + w * (r * r).
 * counts[2i] (+)= spp, counts[2i + 1] (+)= the back-facing samples (int32; with accumulate = 0 both are overwritten).  One call over
 * a + b samples equals a call over a followed by one over b with sample_offset = a, accumulate = 1, bit for bit.
 * Lookup of point p, unit normal n with {normal_bias, backface_max}: cell and axis weights from p exactly as in mcpt_probe_shade;
 * q = p + normal_bias * n per component.  For the corners in the order (dz, dy, dx) = 000 .. 111: wt = (wz wy) wx; the corner's probe i
 * sits at P; it is dead iff counts[2i] > 0 && (float)counts[2i + 1] > backface_max * (float)counts[2i], and a dead probe has a = 0;
 * else u = P - p, lu = sqrtf(dot(u, u)), cosn = lu > 0 ? dot(u, n) / lu : 1, h = (cosn + 1) * 0.5f, wb = h * h + 0.2f; v = q - P,
 * dist = sqrtf(dot(v, v)), (W, S1, S2) of the texel of v; ch = 1; if W > 0: m = S1 / W, m2 = S2 / W, var = fabsf(m2 - m * m), and if
 * dist > m: dd = dist - m, den = var + dd * dd, ch = den > 0 ? var / den : 0, ch = (ch * ch) * ch; a = (wt * wb) * ch.  A = the sum of
 * a in corner order from 0.  If A > 0: every coefficient is b = sum of a_c * L_c in corner order from 0, and out[ch] =
 * mcpt_sh_irradiance_host(b, n)[ch] / A; otherwise (every corner dead or invisible, or A not a number) out is mcpt_probe_shade's value
 * for the same inputs.  weight_out[i] = A (nullable).
 *
 * mcpt_query_probe_depth is enqueued on hip_stream without a synchronisation, through the staging buffers of the ray queries and under
 * their protocol (mcpt_query_closest): info->grew is 0 in the steady state; rays are staged in chunks of at most MCPT_QUERY_CHUNK, whole
 * probes or whole 64-sample blocks of one probe, and the result does not depend on it.  It sees the live scene as it is now.
 * mcpt_probe_shade_visible is enqueued like mcpt_probe_shade.  mcpt_bake_probe_volume runs mcpt_bake_probe_grid, then
 * mcpt_query_probe_depth on the same scene-owned points, and equals the two bit for bit.
 * MCPT_ERR_ARG before any device work: a null scene, params, options or output; n < 0 or n > (2^31 - 1) / 192 (a grid: more probes than
 * that); spp <= 0, sample_offset < 0, or sample_offset + spp > 2^31 - 1 (a progressive caller's sample_offset is the count the probe
 * already has, so this is where counts would stop fitting an int32; the host fold checks the counts themselves); accumulate other than 0
 * or 1; max_distance not positive and finite; normal_bias or backface_max negative or not finite; a non-zero reserved word; a pointer
 * that is not memory of the scene's device; the grid refusals of mcpt_probe_shade.  n == 0 is a valid no-op.  No mcpt_group_* form. */
#define MCPT_PROBE_DEPTH_RES 8
typedef struct {
    uint32_t seed;
    int32_t spp, sample_offset, accumulate;
    float max_distance;
    int32_t reserved[3]; /* must be 0 */
} mcpt_probe_depth_params; /* 32 bytes */
typedef struct {
    float normal_bias, backface_max;
    int32_t reserved[2]; /* must be 0 */
} mcpt_probe_visibility; /* 16 bytes */
int mcpt_query_probe_depth(mcpt_scene *scene, const mcpt_probe_depth_params *params, int64_t n, const float *origins /* n*3, device */,
                           float *moments /* n*192, device */, int32_t *counts /* n*2, device */, void *hip_stream,
                           mcpt_query_info *info /* nullable */);
int mcpt_probe_shade_visible(mcpt_scene *scene, const mcpt_probe_grid *grid, const float *sh /* probes*27, device */,
                             const float *moments /* probes*192, device */, const int32_t *counts /* probes*2, device */,
                             const mcpt_probe_visibility *opts, int64_t n, const float *points /* n*3, device */,
                             const float *normals /* n*3, device */, float *out /* n*3, device */, float *weight_out /* n, device, nullable */,
                             void *hip_stream);
int mcpt_bake_probe_volume(mcpt_scene *scene, const mcpt_probe_grid *grid, const mcpt_params *params, const mcpt_probe_depth_params *depth_params,
                           float *sh /* probes*27, device */, float *moments /* probes*192, device */, int32_t *counts /* probes*2, device */,
                           void *hip_stream, mcpt_stats *stats /* nullable */);
/* Host only, no GPU needed: csrc/mcpt_probe_depth.h compiled for the CPU.  mcpt_probe_depth_fold_host folds given samples: dirs n*spp*3,
 * r n*spp, backfacing n*spp (non-zero: back-facing), probe-major in sample order. */
int mcpt_probe_depth_dirs_host(float *dirs /* 64*3 */);
int mcpt_probe_depth_texel_host(int64_t n, const float *v /* n*3 */, int32_t *texel /* n */);
int mcpt_probe_depth_fold_host(int64_t n, int32_t spp, const float *dirs, const float *r, const uint8_t *backfacing, int32_t accumulate,
                               float *moments /* n*192 */, int32_t *counts /* n*2 */);
int mcpt_probe_shade_visible_host(const mcpt_probe_grid *grid, const float *sh, const float *moments, const int32_t *counts,
                                  const mcpt_probe_visibility *opts, int64_t n, const float *points, const float *normals, float *out,
                                  float *weight_out /* nullable */);

/* ---- Probe-lit frames: a picture of the live scene lit by a baked probe volume, at one closest-hit ray and one grid lookup per camera
 * sample: deterministic for a given seed, free of path noise, and as good as the volume (csrc/mcpt_probes.hip holds the kernels,
 * csrc/mcpt_render.hip the pass).  Float32 in the written order, no FMA.
 *
 * Sample k of pixel m is the feature sample of mcpt_render_aovs_features with the same seed, aov_spp, specular_depth and centre: the same
 * first ray and the same chain steps 1-5, which give the throughput thr, the ray (o, d) of its last segment, and at a hit the double t,
 * p = o + d * (float)t, the shading normal n as stored (not flipped), the uv and the material.  Where that sample would record, the lit
 * sample takes a value v[c]:
 *   miss:     v[c] = thr[c] * sample_env(d)[c]  (the environment map or the background, as mcpt_sample_env gives it for d)
 *   emitter:  v[c] = thr[c] * clampf(0, 1, emit[c] * fabsf(dot(-d, n))), the depth-0 rule of Scene::castRay, here at every chain depth:
 *             an emitter seen in a mirror shows as the emitter.  (The reference shows the sky in its place; that is deliberately not
 *             reproduced.)
 *   other:    a[c] = thr[c] * alb[c], the product the AOV record stores (alb: the conductor reflectance at uv, 1 for dielectrics);
 *             nf = dot(n, d) > 0 ? -n : n;  E = mcpt_probe_shade_visible's value for (p, nf) with volume->visibility when moments are
 *             given, else mcpt_probe_shade's;  v[c] = a[c] * fmaxf(E[c], 0.f)  (the truncated series can ring negative, a picture cannot).
 * Fold per pixel, in sample order:  lit[3m + c]: acc = 0; acc += v_k[c] / (float)aov_spp.  position[3m + ..] (nullable): the sum of p over
 * the samples that ended on a hit (emitters included) divided by their number, 0 without one.  No pixel is sky-culled.
 *
 * The call works on hip_stream and blocks until the outputs are complete, like mcpt_bake_lightmap.  It sees the live scene as it is now
 * and changes no scene state that a later render, query or sequence can observe; it works in the wavefront workspace when a render has
 * left one (info->in_workspace), else in buffers of its own; the scene keeps two eight-byte counters from its first such call on, which no
 * other call reads or reports.  info->chunks: chunks of whole pixels the frame was cut into;
 * info->samples = width * height * aov_spp; info->lookups: samples that ended on a hit that is not an emitter.
 * MCPT_ERR_ARG before any device work: a null scene, camera, opts, volume, outputs, lit, grid or sh; aov_spp outside 0..65536,
 * specular_depth outside 0..8, centre other than 0 or 1, centre 1 with aov_spp > 1; a non-zero reserved word or pointer; moments, counts
 * and visibility not all null or all non-null; a frame mcpt_render_aovs refuses; every grid and visibility refusal of
 * mcpt_probe_shade_visible (with moments null the grid may hold (2^31 - 1) / 27 probes, as for mcpt_probe_shade); a buffer that is not
 * memory of the scene's device.  No mcpt_group_* form. */
typedef struct {
    int32_t aov_spp;        /* camera samples per pixel, 0 => 1, at most 65536; with centre 1: 0 or 1 */
    int32_t specular_depth; /* 0..8, the chains of mcpt_render_aovs_ex */
    int32_t centre;         /* 0 | 1, the centre rays of mcpt_feature_opts */
    uint32_t seed;          /* ignored with centre 1 */
    int32_t reserved[4];    /* must be 0 */
} mcpt_lit_opts;            /* 32 bytes */
typedef struct {            /* device memory of the scene's device, as the probe calls take it */
    const mcpt_probe_grid *grid;             /* host struct */
    const float *sh;                         /* probes*27 */
    const float *moments;                    /* probes*192, nullable: null => the plain lookup (mcpt_probe_shade) */
    const int32_t *counts;                   /* probes*2, null iff moments is null */
    const mcpt_probe_visibility *visibility; /* host struct, null iff moments is null */
} mcpt_probe_volume;        /* 40 bytes */
typedef struct {            /* device memory */
    float *lit;             /* W*H*3, required */
    float *position;        /* W*H*3, nullable */
    void *reserved[2];      /* must be null */
} mcpt_lit_outputs;         /* 32 bytes */
typedef struct {
    int32_t chunks, in_workspace;
    int64_t samples, lookups;
    double ms_total;        /* host wall clock of the call */
} mcpt_lit_info;            /* 32 bytes */
int mcpt_render_probe_lit(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_lit_opts *opts, const mcpt_probe_volume *volume,
                          const mcpt_lit_outputs *outputs, void *hip_stream, mcpt_lit_info *info /* nullable */);

/* ---- The sampled direct term: the light that reaches a Lambertian point straight from the emitters, by light samples and shadow rays,
 * for points that already sit in the memory of the scene's device (csrc/mcpt_direct.h states the arithmetic once for host and device;
 * float32 in the written order, no FMA).  It is the part of Scene::directLighting a Lambertian preview needs, and the complement of a
 * probe volume: the order-2 series of a probe cannot hold a contact shadow, a shadow ray can.
 *
 * D(seed, key_pixel, key_sample, N; p, nf)[c] is E_direct / pi at the point p with unit normal nf.  dot, norm and normalized are those of
 * the render loop (a three-term dot is a.x * b.x + (a.y * b.y + a.z * b.z); normalized leaves a zero vector unchanged), EPS = 1e-4f.
 *   If the scene's light table is empty: D = 0, and no ray is traced.
 *   q = p + nf * EPS per component (Scene.cpp:114, with the normal that faces the viewer).
 *   acc[c] = 0; for j = 0 .. N - 1 in order:
 *     u = the four uniforms of the Philox block with key (seed, key_pixel) and counter (key_sample, depth 0, block j, stream 5)
 *         (mcpt_rng_uniforms_host; streams 0..2 are the channel paths, 3 the camera, 4 the sensors);
 *     (x_l, n_l, emit, pdf) = the scene's light sample for u: the ten floats of mcpt_debug_scene kind 0, the reference's quirks included
 *         (the biased triangle pick inside a mesh light, BVH.cpp:132; a sphere emitter's sample carries emission 0);
 *     w = x_l - q; dist = norm(w); ws = normalized(w); cs = dot(ws, nf); cl = dot(-ws, n_l); g = ((cs * cl) / (dist * dist)) / pdf;
 *     live = cs > 0 && cl > 0 && g <= FLT_MAX  (a NaN fails, and so does a zero distance); a sample that is not live traces no ray;
 *     visible = live && the closest hit of the ray (q, ws) exists with fabs(t - (double)dist) < (double)EPS, t the double of
 *         mcpt_intersect (Scene.cpp:72-75);
 *     if visible: acc[c] = acc[c] + (emit[c] * g) / (float)N.
 *   D[c] = acc[c] / pi (the float pi of the render loop).
 *
 * mcpt_query_direct: out[3i + c] = D(seed, i, key_sample, n_samples; points[i], normals[i])[c].  The call is enqueued on hip_stream
 * without a synchronisation, through the staging buffers of the ray queries and under their protocol (mcpt_query_closest): the buffers
 * are the scene's and only grow, info->grew is 0 in the steady state; the light samples are staged in chunks of at most MCPT_QUERY_CHUNK,
 * whole points or runs of one point's samples, and the result does not depend on it; the scene's query event is recorded behind the
 * call, so an edit issued after it waits.  Only the shadow rays of live samples are traced.  It sees the live scene as it is now.
 * MCPT_ERR_ARG before any device work, with out and info untouched: a null scene or opts; n_samples outside 1..4096; a non-zero reserved
 * word; n < 0 or n * n_samples > 2^31 - 1; n > 0 with a null points, normals or out, or with one that is not memory of the scene's
 * device.  n == 0 is a valid no-op.  No mcpt_group_* form. */
typedef struct {
    uint32_t seed;
    int32_t n_samples;   /* 1..4096 light samples per point */
    uint32_t key_sample; /* the sample word of the Philox counter */
    int32_t reserved[5]; /* must be 0 */
} mcpt_direct_opts;      /* 32 bytes */
int mcpt_query_direct(mcpt_scene *scene, const mcpt_direct_opts *opts, int64_t n, const float *points /* n*3, device */,
                      const float *normals /* n*3, device */, float *out /* n*3, device */, void *hip_stream,
                      mcpt_query_info *info /* nullable */);
/* Host only, no GPU needed.  mcpt_rng_uniforms_host: the Philox block of key (seed, pixel) and counter (sample[i], depth[i], block[i],
 * stream[i]) as four uniforms in [0, 1) per row, as every kernel draws them.  mcpt_direct_samples_host: the geometry of N light samples
 * per point, point-major (light_rows: the ten floats of mcpt_debug_scene kind 0 per sample) -> the shadow ray's origin q and direction
 * ws, dist, live (0 | 1) and contrib = (emit * g) / N, which is 0 where live is 0.  mcpt_direct_fold_host: D from the contributions and
 * the visibility of every sample (non-zero: visible).  MCPT_ERR_ARG: N outside 1..4096, n < 0 or n * N > 2^31 - 1, a null pointer
 * with n > 0. */
int mcpt_rng_uniforms_host(uint32_t seed, uint32_t pixel, int64_t n, const uint32_t *sample, const uint32_t *depth, const uint32_t *block,
                           const uint32_t *stream, float *out /* n*4 */);
int mcpt_direct_samples_host(int64_t n, int32_t N, const float *points /* n*3 */, const float *normals /* n*3 */,
                             const float *light_rows /* n*N*10 */, float *q_out /* n*N*3 */, float *ws_out /* n*N*3 */,
                             float *dist_out /* n*N */, uint8_t *live_out /* n*N */, float *contrib_out /* n*N*3 */);
int mcpt_direct_fold_host(int64_t n, int32_t N, const float *contrib /* n*N*3 */, const uint8_t *visible /* n*N */, float *out /* n*3 */);

/* ---- Indirect-only probes: the volume that goes with the sampled direct term.  The _ex forms take the arguments of mcpt_query_probes,
 * mcpt_bake_probe_grid and mcpt_bake_probe_volume and one option struct; opts null or zeroed gives the plain call bit for bit.
 * indirect_only = 1: in the projection, and in radiance and variance, the value v(i, k, c) of every sample whose first ray
 * mcpt_probe_rays(i, sample_offset + k) has its closest hit on an emitting primitive is replaced by 0.f (the plain call records the
 * depth-0 rule clamp(0, 1, emission * |cos|) there, which is direct light, and clamped).  Everything else is unchanged: a miss keeps the
 * sky, the fold order is the same, accumulate / spp_total compose the same way, and the depth maps of mcpt_bake_probe_volume_ex are
 * those of mcpt_bake_probe_volume.  The switch is a compile-time flavour of the sensor kernels' first-hit code (k_sensor_primary_indirect,
 * csrc/mcpt_kernels.hip); the render loop's kernels do not carry it.
 * MCPT_ERR_ARG besides the plain calls' refusals: indirect_only other than 0 or 1, a non-zero reserved word.  No mcpt_group_* form. */
typedef struct {
    int32_t indirect_only; /* 0 | 1 */
    int32_t reserved[7];   /* must be 0 */
} mcpt_probe_opts;         /* 32 bytes */
int mcpt_query_probes_ex(mcpt_scene *scene, const mcpt_params *params, int64_t n, const float *origins /* n*3, device */,
                         const mcpt_probe_outputs *out, void *hip_stream, mcpt_stats *stats /* nullable */, const mcpt_probe_opts *opts /* nullable */);
int mcpt_bake_probe_grid_ex(mcpt_scene *scene, const mcpt_probe_grid *grid, const mcpt_params *params, float *sh /* probes*27, device */,
                            void *hip_stream, mcpt_stats *stats /* nullable */, const mcpt_probe_opts *opts /* nullable */);
int mcpt_bake_probe_volume_ex(mcpt_scene *scene, const mcpt_probe_grid *grid, const mcpt_params *params, const mcpt_probe_depth_params *depth_params,
                              float *sh /* probes*27, device */, float *moments /* probes*192, device */, int32_t *counts /* probes*2, device */,
                              void *hip_stream, mcpt_stats *stats /* nullable */, const mcpt_probe_opts *opts /* nullable */);

/* ---- Probe-lit frames with direct light: mcpt_render_probe_lit with the sampled direct term added at every surface sample, so that a
 * preview shows contact shadows under moved, deformed and added objects.  Meant for an indirect-only volume (above); with a full volume
 * the direct light is counted twice.  direct null or n_samples == 0 gives mcpt_render_probe_lit bit for bit, info included.  Otherwise
 * only the surface samples ("other" in the rule of mcpt_render_probe_lit) change:
 *   v[c] = a[c] * (fmaxf(E[c], 0.f) + D(direct->seed, m, k, n_samples; p, nf)[c])
 * with m the pixel, k the sample's index within the pixel and p, nf, a the sample's own; direct->seed is used with centre = 1 as well.  At
 * the end of a mirror or glass chain the term is applied like the lookup, with thr inside a.  Sky and emitter samples, the fold,
 * position, info->samples and info->lookups are unchanged.  dinfo->light_samples = lookups * n_samples; dinfo->shadow_rays: the live
 * light samples, each of which traced one shadow ray; dinfo->pieces: the pieces the light samples of the chunks were staged in (a chunk's
 * n * n_samples light samples can exceed its ray arrays; the result does not depend on the cut).  The call blocks, changes nothing a
 * later render, query or sequence can observe, and a second call allocates nothing; the scene's counter of mcpt_render_probe_lit is
 * sixteen bytes.  MCPT_ERR_ARG before any device work, with the outputs, info and dinfo untouched: every refusal of
 * mcpt_render_probe_lit; n_samples outside 0..4096; a non-zero reserved word of direct.  No mcpt_group_* form. */
typedef struct {
    int32_t n_samples;   /* 0 = off, else 1..4096 light samples per surface sample */
    uint32_t seed;
    int32_t reserved[6]; /* must be 0 */
} mcpt_lit_direct_opts;  /* 32 bytes */
typedef struct {
    int64_t light_samples, shadow_rays;
    int32_t pieces;
    int32_t reserved[3];
} mcpt_lit_direct_info;  /* 32 bytes */
int mcpt_render_probe_lit_direct(mcpt_scene *scene, const mcpt_camera *camera, const mcpt_lit_opts *opts,
                                 const mcpt_lit_direct_opts *direct /* nullable */, const mcpt_probe_volume *volume, const mcpt_lit_outputs *outputs,
                                 void *hip_stream, mcpt_lit_info *info /* nullable */, mcpt_lit_direct_info *dinfo /* nullable */);

/* ---- Relighting a probe volume from itself: one bounce of light gathered at every probe of a grid from the previous volume plus
 * sampled direct light, blended into the probe with a hysteresis.  One closest-hit ray per probe sample instead of a path: iterating
 * the update gives multi-bounce indirect light, and the volume follows mcpt_scene_update / _deform / _add_objects / _set_materials /
 * _set_visibility frame by frame (csrc/mcpt_probe_relight.h states the fold and the blend once for host and device; csrc/mcpt_probes.hip
 * holds the kernels).  Float32 in the written order, no FMA.  The probes are the grid's, at the scene-owned points of
 * mcpt_bake_probe_grid.
 *
 * Sample k of probe i is the lit sample of mcpt_render_probe_lit_direct at specular_depth 0 with thr = 1: its first ray is
 * mcpt_probe_rays(seed, i, sample_offset + k), with origin the probe and direction d, and its value v is
 *   miss:     v = sample_env(d)
 *   emitter:  indirect_only 0: v[c] = clampf(0, 1, emit[c] * fabsf(dot(-d, n)));  indirect_only 1: v = 0.f
 *   other:    v[c] = alb[c] * (fmaxf(E[c], 0.f) + D[c]), with p, nf and alb exactly as in the lit rule, E the lookup of (p, nf) in
 *             `volume` (mcpt_probe_shade when volume->moments is null, else mcpt_probe_shade_visible with volume->visibility) and
 *             D = D(direct_seed, key pixel i, key sample sample_offset + k, direct_samples; p, nf), mcpt_query_direct's term; D is 0
 *             with direct_samples == 0 or an empty light table, and no shadow ray is traced then.
 * Surfaces are treated as Lambertian with the AOV albedo (dielectrics 1, conductors their reflectance): the lit pass's approximation.
 * Fold:   fresh[27i + 3j + c]: acc = 0; for k in sample order acc = acc + (v_k[c] * (kFourPi * Y_j(d_k))) / (float)spp, which is
 *         mcpt_query_probes' projection with spp_total = spp and accumulate = 0.
 * Blend:  hysteresis == 0: out->sh = fresh; otherwise out->sh = hysteresis * volume->sh + (1.f - hysteresis) * fresh, two products and
 *         one sum.  volume->sh is never written.
 * Depth (optional): when out->moments is given, moments and counts are what mcpt_query_probe_depth{seed, spp, sample_offset,
 *         accumulate = 0, max_distance} gives for the same points, bit for bit, from the same traced hits (no second trace).  A limit:
 *         depth is not blended, the maps are those of this call's samples alone.
 * Use with a split volume: for a volume baked with indirect_only, call with indirect_only = 1 and direct_samples > 0; for a full volume
 * with both 0.  The other two combinations are legal: indirect_only = 0 with direct_samples > 0 counts direct light twice,
 * indirect_only = 1 with direct_samples = 0 not at all.
 *
 * Protocol, as mcpt_query_probe_depth and mcpt_query_direct: the call is enqueued on hip_stream without a host synchronisation, through
 * the staging buffers of the ray queries; info->grew is 0 and nothing is allocated on a second call of the same size; the scene's query
 * event is recorded behind it, so an edit issued afterwards waits.  Probe rays are staged in chunks of at most MCPT_QUERY_CHUNK, whole
 * probes or whole 64-sample blocks of one probe, and the result does not depend on the cut: a probe whose samples span pieces passes its
 * partial sums through out->sh and blends at its last piece.  The per-sample records, D and the shadow-ray staging live in scene-owned
 * buffers that only grow and are counted by mcpt_scene_probe_buffers.
 * MCPT_ERR_ARG before any device work, with the outputs and info untouched: a null scene, volume, opts, out or out->sh; every grid,
 * visibility and all-or-none refusal of mcpt_render_probe_lit; spp < 1, sample_offset < 0 or sample_offset + spp > 2^31 - 1; hysteresis
 * outside [0, 1) or not a number; indirect_only other than 0 or 1; direct_samples outside 0..4096; max_distance not positive and finite
 * while depth outputs are given; out->moments and out->counts not both null or both non-null; a non-zero reserved word or pointer;
 * probes * spp or probes * spp * direct_samples beyond 2^31 - 1; out->sh overlapping volume->sh, or out->moments / out->counts
 * overlapping the volume's; a pointer that is not memory of the scene's device.  No mcpt_group_* form. */
typedef struct {
    uint32_t seed;            /* probe rays: mcpt_probe_rays(seed, i, sample_offset + k) */
    int32_t  spp;             /* >= 1 probe rays per probe */
    int32_t  sample_offset;   /* >= 0, sample_offset + spp <= 2^31 - 1 */
    float    hysteresis;      /* 0 <= h < 1: share of the previous coefficients kept */
    int32_t  indirect_only;   /* 0 | 1: a probe ray that ends on an emitter records 0 */
    int32_t  direct_samples;  /* 0 = off, else 1..4096 light samples per surface hit */
    uint32_t direct_seed;
    float    max_distance;    /* read only when depth outputs are given: positive, finite */
    int32_t  reserved[8];     /* must be 0 */
} mcpt_probe_relight_opts;    /* 64 bytes */
typedef struct {              /* device memory */
    float   *sh;              /* probes*27, required; must not overlap volume->sh */
    float   *moments;         /* probes*192, nullable */
    int32_t *counts;          /* probes*2, null iff moments is null */
    void    *reserved;        /* must be null */
} mcpt_probe_relight_outputs; /* 32 bytes */
int mcpt_probe_volume_relight(mcpt_scene *scene, const mcpt_probe_volume *volume /* the previous volume, read only */,
                              const mcpt_probe_relight_opts *opts, const mcpt_probe_relight_outputs *out, void *hip_stream,
                              mcpt_query_info *info /* nullable */);
/* Host only, no GPU needed: the projection fold and the blend of csrc/mcpt_probe_relight.h compiled for the CPU.  dirs and values are
 * n*spp*3, probe-major in sample order.  MCPT_ERR_ARG: n < 0 or n > (2^31 - 1) / 27, spp < 1, hysteresis outside [0, 1), a null dirs,
 * values or out with n > 0, a null prev with hysteresis != 0. */
int mcpt_probe_relight_fold_host(int64_t n, int32_t spp, const float *dirs /* n*spp*3 */, const float *values /* n*spp*3 */,
                                 float hysteresis, const float *prev /* n*27, nullable iff hysteresis == 0 */, float *out /* n*27 */);

const char *mcpt_last_error(void);
const char *mcpt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MCPT_H */
