"""ctypes binding to libmcpt_hip.so (the C ABI of include/mcpt.h) and a Python mirror of the reference's
`Renderer` seam: `HipScene` plays Scene (after Add/buildBVH), `HipScene.render` plays Renderer::Render
(reference src/Renderer.hpp:16-22, src/Scene.hpp:104-131).

There is no CPU fallback here: if the HIP library is missing or no GPU is usable, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCPT_LIB") or os.path.join(HERE, "libmcpt_hip.so")  # MCPT_LIB: diagnostic builds only
CHECK_LIB_PATH = os.path.join(HERE, "libmcpt_hip_check.so")  # the checking build (build.build_check); tests only

EXPORTS = ["mcpt_scene_create", "mcpt_scene_destroy", "mcpt_render", "mcpt_render_device", "mcpt_render_adaptive", "mcpt_render_aovs",
           "mcpt_render_aovs_ex", "mcpt_denoise", "mcpt_render_denoised", "mcpt_intersect",
           "mcpt_cast_rays", "mcpt_camera_rays", "mcpt_scene_get_info", "mcpt_bvh_dump", "mcpt_scene_create_ex", "mcpt_scene_dump_bvh", "mcpt_tonemap", "mcpt_tonemap_device", "mcpt_debug_fmath", "mcpt_debug_material", "mcpt_debug_scene", "mcpt_debug_shadow", "mcpt_debug_counters",
           "mcpt_cull_bound", "mcpt_debug_classify",
           "mcpt_scene_update", "mcpt_group_update", "mcpt_transform_triangles",
           "mcpt_scene_deform", "mcpt_group_deform", "mcpt_deform_triangles",
           "mcpt_scene_set_materials", "mcpt_scene_set_environment", "mcpt_group_set_materials", "mcpt_group_set_environment",
           "mcpt_scene_set_visibility", "mcpt_scene_get_visibility", "mcpt_group_set_visibility", "mcpt_compact_scene",
           "mcpt_scene_add_objects", "mcpt_group_add_objects", "mcpt_extend_scene",
           "mcpt_scene_snapshot", "mcpt_render_motion", "mcpt_temporal_blend", "mcpt_temporal_accumulate",
           "mcpt_temporal_accumulate_ex",
           "mcpt_sequence_create", "mcpt_sequence_frame", "mcpt_sequence_reset", "mcpt_sequence_destroy",
           "mcpt_sequence_create_ex", "mcpt_sequence_flags",
           "mcpt_temporal_history_len", "mcpt_render_adaptive_guided", "mcpt_render_adaptive_denoised",
           "mcpt_sequence_create_adaptive", "mcpt_sequence_counts",
           "mcpt_render_motion_ex", "mcpt_sequence_create_motion",
           "mcpt_temporal_accumulate_weighted", "mcpt_temporal_history_weight", "mcpt_render_adaptive_weighted",
           "mcpt_sequence_create_weighted", "mcpt_sequence_weight",
           "mcpt_temporal_accumulate_moments", "mcpt_moments_variance", "mcpt_sequence_create_moments", "mcpt_sequence_moments",
           "mcpt_centre_rays", "mcpt_render_aovs_features", "mcpt_render_motion_features", "mcpt_sequence_create_features",
           "mcpt_denoise_feedback", "mcpt_sequence_create_feedback", "mcpt_sequence_history",
           "mcpt_scene_ray_counts", "mcpt_scene_primary_conductor_counts",
           "mcpt_query_closest", "mcpt_query_occluded", "mcpt_query_radiance", "mcpt_sensor_rays",
           "mcpt_lightmap_texels", "mcpt_lightmap_scatter", "mcpt_bake_lightmap", "mcpt_lightmap_texels_host", "mcpt_lightmap_dilate_host",
           "mcpt_query_probes", "mcpt_probe_rays", "mcpt_probe_shade", "mcpt_bake_probe_grid", "mcpt_scene_probe_buffers",
           "mcpt_sh_basis_host", "mcpt_sh_irradiance_host", "mcpt_probe_grid_points_host", "mcpt_probe_shade_host",
           "mcpt_query_probe_depth", "mcpt_probe_shade_visible", "mcpt_bake_probe_volume",
           "mcpt_probe_depth_dirs_host", "mcpt_probe_depth_texel_host", "mcpt_probe_depth_fold_host", "mcpt_probe_shade_visible_host",
           "mcpt_render_probe_lit",
           "mcpt_query_probes_ex", "mcpt_bake_probe_grid_ex", "mcpt_bake_probe_volume_ex", "mcpt_render_probe_lit_direct",
           "mcpt_query_direct", "mcpt_rng_uniforms_host", "mcpt_direct_samples_host", "mcpt_direct_fold_host",
           "mcpt_probe_volume_relight", "mcpt_probe_relight_fold_host",
           "mcpt_group_create", "mcpt_group_render", "mcpt_group_size", "mcpt_group_get_info", "mcpt_group_scene", "mcpt_group_destroy", "mcpt_group_last_error",
           "mcpt_last_error", "mcpt_version"]


class McptError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("mcpt error %d: %s" % (code, msg))
        self.code = code


class SceneDesc(C.Structure):
    _fields_ = [("n_objects", C.c_int32), ("n_triangles", C.c_int32), ("n_materials", C.c_int32),
                ("env_w", C.c_int32), ("env_h", C.c_int32), ("background", C.c_float * 3),
                ("objects", C.c_void_p), ("triangles", C.c_void_p), ("materials", C.c_void_p), ("env_pixels", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [("spp", C.c_int32), ("spp_total", C.c_int32), ("sample_offset", C.c_int32), ("rr_rate", C.c_float),
                ("n_dir_sample", C.c_int32), ("enable_shadow", C.c_int32), ("seed", C.c_uint32), ("accumulate", C.c_int32),
                ("tile_size", C.c_int32), ("rank", C.c_int32), ("nranks", C.c_int32), ("spp_per_pass", C.c_int32),
                ("pool_paths", C.c_int32), ("max_depth", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("paths", C.c_uint64), ("vertices", C.c_uint64), ("shaded", C.c_uint64),
                ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("ref_scene_rays", C.c_uint64),
                ("iterations", C.c_uint64), ("overflow_paths", C.c_uint64), ("ms_total", C.c_double),
                ("ms_trace_closest", C.c_double), ("ms_trace_shadow", C.c_double), ("ms_shade", C.c_double),
                ("ms_generate", C.c_double), ("ms_resolve", C.c_double),
                ("n_trace_closest", C.c_uint64), ("n_trace_shadow", C.c_uint64), ("n_shade", C.c_uint64),
                ("n_generate", C.c_uint64), ("n_resolve", C.c_uint64), ("ms_direct", C.c_double), ("n_direct", C.c_uint64), ("direct_vertices", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Adaptive(C.Structure):
    _fields_ = [("min_spp", C.c_int32), ("dilate", C.c_int32), ("threshold", C.c_float), ("rel_floor", C.c_float), ("reserved", C.c_int32 * 4)]


class AdaptiveInfo(C.Structure):
    _fields_ = [("rounds", C.c_int32), ("reserved", C.c_int32), ("active_pixels", C.c_uint64 * 16), ("ms_round", C.c_double * 16)]

    def as_dict(self):
        n = self.rounds
        return {"rounds": n, "active_pixels": [int(x) for x in self.active_pixels[:n]], "ms_round": [float(x) for x in self.ms_round[:n]]}


class DenoiseOpts(C.Structure):
    _fields_ = [("aov_spp", C.c_int32), ("iterations", C.c_int32), ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float),
                ("specular_depth", C.c_int32), ("reserved", C.c_int32 * 2)]


class DenoiseInfo(C.Structure):
    _fields_ = [("ms_render", C.c_double), ("ms_aov", C.c_double), ("ms_denoise", C.c_double), ("ms_total", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def denoise_opts(aov_spp=0, iterations=0, sigma_l=0.0, sigma_n=0.0, sigma_z=0.0, specular_depth=0):
    """mcpt_denoise_opts (0 = the library's default for every field; specular_depth 0: first-hit AOVs)."""
    return DenoiseOpts(aov_spp=int(aov_spp), iterations=int(iterations), sigma_l=float(sigma_l), sigma_n=float(sigma_n), sigma_z=float(sigma_z),
                       specular_depth=int(specular_depth))


class TemporalOpts(C.Structure):
    _fields_ = [("max_history", C.c_int32), ("depth_tol", C.c_float), ("reserved", C.c_int32 * 6)]


def temporal_opts(max_history=0, depth_tol=0.0):
    """mcpt_temporal_opts (0 = the library's default: a history of at most 32 frames, a relative depth tolerance of 0.02)."""
    return TemporalOpts(max_history=int(max_history), depth_tol=float(depth_tol))


class HistoryOpts(C.Structure):
    _fields_ = [("normal_test", C.c_int32), ("color_clamp", C.c_int32), ("normal_min", C.c_float), ("clamp_k", C.c_float), ("reserved", C.c_int32 * 4)]


def history_opts(normal_test=False, color_clamp=False, normal_min=0.0, clamp_k=0.0):
    """mcpt_history_opts: the normal test on every tap and the neighbourhood colour clamp of the reprojected history, both off by default
    (normal_min, clamp_k 0 = the library's defaults 0.9 and 1)."""
    return HistoryOpts(normal_test=int(normal_test), color_clamp=int(color_clamp), normal_min=float(normal_min), clamp_k=float(clamp_k))


FLAG_NORMAL, FLAG_CLAMP = 1, 2  # the bits of a history-rejection flags byte


class SequenceOpts(C.Structure):
    _fields_ = [("temporal", TemporalOpts), ("denoise", DenoiseOpts), ("filter", C.c_int32), ("reserved", C.c_int32 * 7)]


SEQUENCE_OUTPUTS = ("fb", "accumulated", "denoised", "variance", "len", "aov", "motion", "rgba")  # mcpt_sequence_outputs, in its order


class SequenceOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in SEQUENCE_OUTPUTS]


class SequenceInfo(C.Structure):
    _fields_ = [("ms_render", C.c_double), ("ms_aov", C.c_double), ("ms_motion", C.c_double), ("ms_accumulate", C.c_double),
                ("ms_filter", C.c_double), ("ms_total", C.c_double), ("frame_index", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class SequenceAdaptive(C.Structure):
    _fields_ = [("rule", Adaptive), ("guided", C.c_int32), ("reserved", C.c_int32 * 7)]


def sequence_adaptive(min_spp, threshold, rel_floor=1e-3, dilate=1, guided=False):
    """mcpt_sequence_adaptive: the rule of render_adaptive for every frame of a sequence (each frame's `spp` is the cap); guided: the
    threshold of a pixel is scaled by sqrt(the history length it is about to get)."""
    return SequenceAdaptive(rule=Adaptive(min_spp=int(min_spp), dilate=int(dilate), threshold=float(threshold), rel_floor=float(rel_floor)),
                            guided=int(guided))


class SequenceMotion(C.Structure):
    _fields_ = [("specular_motion", C.c_int32), ("reserved", C.c_int32 * 7)]


class SequenceWeighted(C.Structure):
    _fields_ = [("weighted", C.c_int32), ("reserved", C.c_int32 * 7)]


class MomentsOpts(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("min_len", C.c_int32), ("radius", C.c_int32), ("sigma_z", C.c_float), ("reserved", C.c_int32 * 4)]


def moments_opts(enabled=True, min_len=0, radius=0, sigma_z=0.0):
    """mcpt_moments_opts: the variance of a sequence from the temporal moments of its luminance.  min_len: the shortest history whose
    variance is temporal (0: 4); radius, sigma_z: the window and the depth gate of the spatial estimate shorter histories get (0: 3, 1)."""
    return MomentsOpts(enabled=int(bool(enabled)), min_len=int(min_len), radius=int(radius), sigma_z=float(sigma_z))


class FeatureOpts(C.Structure):
    _fields_ = [("centre", C.c_int32), ("reserved", C.c_int32 * 7)]


class FeedbackOpts(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("reserved", C.c_int32 * 7)]


assert C.sizeof(FeedbackOpts) == 32
assert C.sizeof(SequenceMotion) == 32 and C.sizeof(SequenceWeighted) == 32 and C.sizeof(MomentsOpts) == 32 and C.sizeof(FeatureOpts) == 32
assert C.sizeof(Adaptive) == 32 and C.sizeof(AdaptiveInfo) == 264 and C.sizeof(SequenceAdaptive) == 64
assert C.sizeof(TemporalOpts) == 32 and C.sizeof(DenoiseOpts) == 32 and C.sizeof(HistoryOpts) == 32  # the sizes include/mcpt.h states
assert C.sizeof(SequenceOpts) == 96 and C.sizeof(SequenceOutputs) == 64 and C.sizeof(SequenceInfo) == 64


class BuildOptions(C.Structure):
    _fields_ = [("builder", C.c_int32), ("quantise", C.c_int32), ("instancing", C.c_int32), ("reserved", C.c_int32 * 5)]


BUILDERS = {"default": 0, "sah": 1, "reference": 2, "lbvh": 3, "ploc": 4}  # MCPT_BUILD_*


class SceneInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("bvh_height", C.c_int32), ("n_lights", C.c_int32), ("n_prims", C.c_int32),
                ("scene_bytes", C.c_uint64), ("build_ms", C.c_double), ("upload_ms", C.c_double), ("builder", C.c_int32),
                ("quantised", C.c_int32), ("n_instances", C.c_int32), ("lds_resident", C.c_int32), ("init_ms", C.c_double)]


class GroupInfo(C.Structure):
    _fields_ = [("n_devices", C.c_int32), ("uses_rccl", C.c_int32), ("build_ms", C.c_double), ("upload_ms_max", C.c_double),
                ("init_ms_max", C.c_double), ("setup_ms", C.c_double)]


class ObjectTransform(C.Structure):
    _fields_ = [("object", C.c_int32), ("m", C.c_float * 12)]


class UpdateInfo(C.Structure):
    _fields_ = [("path", C.c_int32), ("n_moved_tris", C.c_int32), ("transform_ms", C.c_double), ("build_ms", C.c_double),
                ("upload_ms", C.c_double), ("total_ms", C.c_double), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        """path 0: host rebuild, 1: device rebuild, 2: in place (set_materials / set_environment)."""
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "reserved"}


class Material(C.Structure):
    _fields_ = [("type", C.c_int32), ("textured", C.c_int32), ("roughness", C.c_float), ("iorA", C.c_float), ("iorB", C.c_float),
                ("base_reflectance", C.c_float * 3), ("emission", C.c_float * 3)]


class MaterialEdit(C.Structure):
    _fields_ = [("index", C.c_int32), ("material", Material)]


class ObjectMaterial(C.Structure):
    _fields_ = [("object", C.c_int32), ("material", C.c_int32)]


class ObjectVisibility(C.Structure):
    _fields_ = [("object", C.c_int32), ("visible", C.c_int32)]


assert C.sizeof(Material) == 44 and C.sizeof(MaterialEdit) == 48 and C.sizeof(ObjectMaterial) == 8 and C.sizeof(ObjectVisibility) == 8


class SceneAddition(C.Structure):
    _fields_ = [("n_objects", C.c_int32), ("n_triangles", C.c_int32), ("n_materials", C.c_int32),
                ("objects", C.c_void_p), ("triangles", C.c_void_p), ("materials", C.c_void_p), ("reserved", C.c_int32 * 4)]


def _addition(sd, objects, triangles, materials):
    """mcpt_scene_addition over arrays with the dtypes of `sd` (objects: first_tri relative to `triangles`, material an index into the
    table after the append); -> (struct, the arrays to keep alive)."""
    def records(x, dtype):  # an array, or a sequence of single records
        if x is None or (not isinstance(x, np.ndarray) and len(x) == 0):
            return np.zeros(0, dtype)
        if not isinstance(x, np.ndarray):
            x = np.stack([np.asarray(r, dtype=dtype).reshape(()) for r in x])
        return np.ascontiguousarray(x, dtype=dtype).reshape(-1)

    obj, tri, mat = records(objects, sd.objects.dtype), records(triangles, sd.triangles.dtype), records(materials, sd.materials.dtype)
    a = SceneAddition()
    a.n_objects, a.n_triangles, a.n_materials = len(obj), len(tri), len(mat)
    a.objects = obj.ctypes.data if len(obj) else None
    a.triangles = tri.ctypes.data if len(tri) else None
    a.materials = mat.ctypes.data if len(mat) else None
    return a, (obj, tri, mat)


def _visibility_items(items):
    """An iterable of (object index, visible) as an array of mcpt_object_visibility.  `visible` is a bool, or the integer to pass as it
    is (the library refuses anything but 0 and 1)."""
    items = list(items)
    arr = (ObjectVisibility * max(len(items), 1))()
    for k, (obj, vis) in enumerate(items):
        arr[k].object, arr[k].visible = int(obj), int(vis)
    return arr, len(items)


def _material_lists(edits, assign):
    """edits: an iterable of (material index, material), a material being one record of scenes.MAT_DTYPE (or anything with its fields);
    assign: an iterable of (object index, material index).  -> (mcpt_material_edit array, n, mcpt_object_material array, n)."""
    edits, assign = list(edits), list(assign)
    ea, aa = (MaterialEdit * max(len(edits), 1))(), (ObjectMaterial * max(len(assign), 1))()
    for k, (idx, m) in enumerate(edits):
        ea[k].index = int(idx)
        mm = ea[k].material
        mm.type, mm.textured = int(m["type"]), int(m["textured"])
        mm.roughness, mm.iorA, mm.iorB = float(m["roughness"]), float(m["iorA"]), float(m["iorB"])
        mm.base_reflectance = (C.c_float * 3)(*[float(x) for x in np.asarray(m["base_reflectance"]).reshape(3)])
        mm.emission = (C.c_float * 3)(*[float(x) for x in np.asarray(m["emission"]).reshape(3)])
    for k, (obj, mat) in enumerate(assign):
        aa[k].object, aa[k].material = int(obj), int(mat)
    return ea, len(edits), aa, len(assign)


def _environment(background, env):
    """(background float[3], env_w, env_h, pixel pointer or None, the array to keep alive)."""
    bg = (C.c_float * 3)(*[float(x) for x in np.asarray(background, dtype=np.float64).reshape(3)])
    if env is None:
        return bg, 0, 0, None, None
    env = np.ascontiguousarray(env, dtype=np.float32)
    if env.ndim != 3 or env.shape[2] != 3 or env.size == 0:
        raise ValueError("set_environment: a map has shape (h, w, 3), not %s" % (env.shape,))
    return bg, int(env.shape[1]), int(env.shape[0]), _ptr(env), env


class CullInfo(C.Structure):
    _fields_ = [("classified", C.c_int32), ("rho", C.c_float), ("scale", C.c_float), ("aspect", C.c_float), ("focal", C.c_float),
                ("lens", C.c_float), ("h", C.c_double), ("s_far", C.c_double), ("reach", C.c_double), ("fmin", C.c_double)]

    def as_dict(self):
        """Floats as numpy float32, so that two records can be compared bit for bit and used in float32 arithmetic as they are."""
        return {k: (np.float32(getattr(self, k)) if t is C.c_float else getattr(self, k)) for k, t in self._fields_}


class ObjectVertices(C.Structure):
    _fields_ = [("object", C.c_int32), ("on_device", C.c_int32), ("positions", C.c_void_p)]


class DevicePositions:
    """Vertex positions that already sit in the memory of the scene's device: the address of n_tri * 9 contiguous float32 values (v0, v1, v2
    of each triangle).  HipScene.deform also takes any object with __cuda_array_interface__, or with data_ptr() and is_cuda (a torch
    tensor), directly."""

    def __init__(self, ptr, n_tri):
        self.ptr, self.n_tri = int(ptr), int(n_tri)
        if self.ptr == 0 or self.n_tri < 0:
            raise ValueError("DevicePositions: a non-null device address and a triangle count >= 0")


# Element types of device buffers: name (numpy's, and the attribute of torch that is its dtype) -> the typestrs of
# __cuda_array_interface__ that mean it, the one a torch tensor of that dtype stands for first.
DTYPES = {"float32": ("<f4", "=f4", "|f4"), "float64": ("<f8", "=f8"), "int32": ("<i4", "=i4"), "uint8": ("|u1", "<u1", "=u1")}


def _device_buffer(v, who, what, dtype="float32"):
    """(address, shape) of a buffer in device memory -- anything with __cuda_array_interface__, or with data_ptr() and is_cuda (a torch
    tensor) -- or None for anything else.  Element type and C-contiguity are checked here (ValueError); the shape is the caller's to check."""
    cai = getattr(v, "__cuda_array_interface__", None)
    if cai is not None:
        shape, typestr, strides = tuple(int(d) for d in cai["shape"]), cai["typestr"], cai.get("strides")
        ptr = cai["data"][0]
    elif hasattr(v, "data_ptr") and getattr(v, "is_cuda", False):
        if not v.is_contiguous():
            raise ValueError("%s: a device tensor must be contiguous" % who)
        name = str(v.dtype).rsplit(".", 1)[-1]
        shape, typestr, strides = tuple(int(d) for d in v.shape), DTYPES.get(name, (name,))[0], None
        ptr = v.data_ptr()
    else:
        return None
    if typestr not in DTYPES[dtype]:
        raise ValueError("%s: %s must be %s, not %s" % (who, what, dtype, typestr))
    if strides is not None:
        want, acc = [], int(typestr[2:])
        for d in reversed(shape):
            want.insert(0, acc)
            acc *= d
        if tuple(strides) != tuple(want):
            raise ValueError("%s: %s must be C-contiguous" % (who, what))
    return int(ptr), shape


def _device_array(who, what, v, shape, dtype="float32"):
    """The address of a C-contiguous device buffer of `dtype` and `shape`; a None in `shape` leaves that extent free (_rows).  ValueError
    for anything that is not a device buffer, and for another element type, layout or shape."""
    b = _device_buffer(v, who, what, dtype)
    if b is None:
        raise ValueError("%s: %s is a buffer in device memory (__cuda_array_interface__, or data_ptr() and is_cuda)" % (who, what))
    if len(b[1]) != len(shape) or any(w is not None and w != d for w, d in zip(shape, b[1])):
        raise ValueError("%s: %s has shape (%s), not %s" % (who, what, ", ".join("n" if w is None else str(w) for w in shape), b[1]))
    return b[0]


def _rows(who, what, v, width):
    """(address, n) of a float32 (n, width) device input: the item count of a call comes from its first input."""
    return _device_array(who, what, v, (None, width)), _device_buffer(v, who, what)[1][0]


def _is_torch(*vs):
    return all(hasattr(v, "data_ptr") and getattr(v, "is_cuda", False) for v in vs)


def _device_of(*vs):
    """The torch device of the first of a call's device inputs when all of them are torch tensors, else None: the call cannot allocate."""
    return vs[0].device if _is_torch(*vs) else None


def _outputs(who, spec, out, device, stream):
    """The output buffers of a call -> (out, {name: address}, stream).  spec: name -> (shape, dtype name), in the call's order; the one
    name None stands for a call whose `out` is a bare buffer, not a dict.  out None: torch.empty tensors on the torch device `device`
    (None: the call cannot allocate, its device inputs are not torch tensors), and the stream then defaults to torch's current one
    there.  Every buffer, allocated or the caller's, passes _device_array."""
    bare = None in spec
    if out is None:
        if device is None:
            raise ValueError("%s: out is required unless the device inputs are torch tensors" % who)
        import torch
        out = {w: torch.empty(shape, dtype=getattr(torch, dt), device=device) for w, (shape, dt) in spec.items()}
        if stream is None:
            stream = torch.cuda.current_stream(device).cuda_stream
        if bare:
            out = out[None]
    bufs, ptrs = ({None: out} if bare else out), {}
    for w, (shape, dt) in spec.items():
        if w not in bufs:
            raise ValueError("%s: out has no buffer for %r" % (who, w))
        ptrs[w] = _device_array(who, "out" if bare else "out[%r]" % w, bufs[w], shape, dt)
    return out, ptrs, stream


def _row_shape(n, width):
    return (n,) if width == 1 else (n, width)


def _device_positions(v):
    """DevicePositions for a device buffer, None for anything else.  Shape, dtype and contiguity are checked here: the library reads
    n_tri * 9 float32 values at the address."""
    if isinstance(v, DevicePositions):
        return v
    b = _device_buffer(v, "deform", "device positions")
    if b is None:
        return None
    ptr, shape = b
    n = 1
    for d in shape:
        n *= int(d)
    if not ((len(shape) == 3 and shape[1:] == (3, 3)) or len(shape) == 1) or n % 9:
        raise ValueError("deform: positions have shape (n_tri, 3, 3) or (n_tri * 9,), not %s" % (shape,))
    return DevicePositions(ptr, n // 9) if n else None


class RayBuffers(C.Structure):
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("tmax", C.c_void_p)]


class HitBuffers(C.Structure):
    _fields_ = [("t", C.c_void_p), ("prim", C.c_void_p), ("object", C.c_void_p), ("uv", C.c_void_p), ("normal", C.c_void_p), ("point", C.c_void_p)]


class QueryInfo(C.Structure):
    _fields_ = [("launches", C.c_int32), ("grew", C.c_int32), ("staged_bytes", C.c_int64), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {"launches": int(self.launches), "grew": int(self.grew), "staged_bytes": int(self.staged_bytes)}


class SensorBuffers(C.Structure):
    _fields_ = [("origins", C.c_void_p), ("dirs", C.c_void_p), ("kind", C.c_int32), ("reserved", C.c_int32 * 3)]


class SensorOutputs(C.Structure):
    _fields_ = [("radiance", C.c_void_p), ("variance", C.c_void_p)]


SENSOR_KINDS = {"ray": 0, "hemisphere": 1}  # MCPT_SENSOR_*


def _sensor_kind(who, kind):
    if not isinstance(kind, str) or kind not in SENSOR_KINDS:
        raise ValueError("%s: kind is one of %s, not %r" % (who, tuple(SENSOR_KINDS), kind))
    return SENSOR_KINDS[kind]


# The outputs of HipScene.query_closest: name -> (element type, values per ray)
QUERY_OUTPUTS = {"t": ("float64", 1), "prim": ("int32", 1), "object": ("int32", 1), "uv": ("float32", 2), "normal": ("float32", 3),
                 "point": ("float32", 3)}


def _query_rays(who, origins, dirs, tmax):
    """The device addresses and the ray count of a query's inputs: float32, C-contiguous, (n, 3) and (n, 3), tmax (n,) or None."""
    bo, bd = _device_buffer(origins, who, "origins"), _device_buffer(dirs, who, "dirs")
    if bo is None or bd is None:
        raise ValueError("%s: origins and dirs are buffers in device memory (__cuda_array_interface__, or data_ptr() and is_cuda)" % who)
    if len(bo[1]) != 2 or bo[1][1] != 3 or bd[1] != bo[1]:
        raise ValueError("%s: origins and dirs have shape (n, 3), not %s and %s" % (who, bo[1], bd[1]))
    n = bo[1][0]
    pt = _device_array(who, "tmax", tmax, (n,)) if tmax is not None else 0
    return n, RayBuffers(bo[0] or None, bd[0] or None, pt or None)


class LightmapDesc(C.Structure):
    _fields_ = [("object", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("flip_normals", C.c_int32), ("reserved", C.c_int32 * 4)]


class LightmapTexelsOut(C.Structure):
    _fields_ = [("texel", C.c_void_p), ("prim", C.c_void_p), ("bary", C.c_void_p), ("origins", C.c_void_p), ("normals", C.c_void_p)]


class LightmapInfo(C.Structure):
    _fields_ = [("n_texels", C.c_int64), ("items", C.c_int64), ("grew", C.c_int32), ("reserved0", C.c_int32), ("ms_texels", C.c_double),
                ("ms_radiance", C.c_double), ("ms_scatter", C.c_double), ("reserved", C.c_int32 * 4)]

    def as_dict(self):
        return {"n_texels": int(self.n_texels), "items": int(self.items), "grew": int(self.grew), "ms_texels": float(self.ms_texels),
                "ms_radiance": float(self.ms_radiance), "ms_scatter": float(self.ms_scatter)}


# The outputs of HipScene.lightmap_texels: name -> (element type, values per texel)
LIGHTMAP_OUTPUTS = {"texel": ("int32", 1), "prim": ("int32", 1), "bary": ("float32", 2), "origins": ("float32", 3), "normals": ("float32", 3)}


def _lightmap_desc(object, width, height, flip_normals=False):
    return LightmapDesc(int(object), int(width), int(height), 1 if flip_normals else 0, (C.c_int32 * 4)(0, 0, 0, 0))


class ProbeGrid(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("spacing", C.c_float * 3), ("dims", C.c_int32 * 3), ("reserved", C.c_int32 * 3)]


class ProbeOutputs(C.Structure):
    _fields_ = [("sh", C.c_void_p), ("radiance", C.c_void_p), ("variance", C.c_void_p), ("reserved", C.c_void_p)]


def _probe_grid(who, origin, spacing, dims):
    """mcpt_probe_grid from three triples; the library's refusals (dims < 1, too many probes, a spacing that is not positive and finite) are
    made here as well, before any buffer is sized from the grid."""
    try:
        o, s = [float(v) for v in origin], [float(v) for v in spacing]
        d = [int(v) for v in dims]
    except (TypeError, ValueError):
        raise ValueError("%s: origin, spacing and dims are triples of numbers" % who)
    if len(o) != 3 or len(s) != 3 or len(d) != 3 or any(int(v) != v for v in dims):
        raise ValueError("%s: origin, spacing and dims are triples (dims of integers)" % who)
    if any(v < 1 for v in d) or d[0] * d[1] * d[2] > (2 ** 31 - 1) // 27:
        raise ValueError("%s: every member of dims is >= 1 and the grid has at most (2^31 - 1) / 27 probes, not %s" % (who, d))
    if any(not (v > 0 and np.isfinite(np.float32(v))) for v in s):
        raise ValueError("%s: spacing is positive and finite, not %s" % (who, s))
    return ProbeGrid((C.c_float * 3)(*o), (C.c_float * 3)(*s), (C.c_int32 * 3)(*d), (C.c_int32 * 3)(0, 0, 0)), d[0] * d[1] * d[2]


class ProbeDepthParams(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("spp", C.c_int32), ("sample_offset", C.c_int32), ("accumulate", C.c_int32), ("max_distance", C.c_float),
                ("reserved", C.c_int32 * 3)]


class ProbeVisibility(C.Structure):
    _fields_ = [("normal_bias", C.c_float), ("backface_max", C.c_float), ("reserved", C.c_int32 * 2)]


class ProbeOpts(C.Structure):
    _fields_ = [("indirect_only", C.c_int32), ("reserved", C.c_int32 * 7)]


def _probe_opts(indirect_only):
    """The options argument of the probe calls' _ex entries: None (the plain call, include/mcpt.h) unless indirect_only is set."""
    return C.byref(ProbeOpts(indirect_only=1)) if indirect_only else None


class LitDirectOpts(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("seed", C.c_uint32), ("reserved", C.c_int32 * 6)]


class LitDirectInfo(C.Structure):
    _fields_ = [("light_samples", C.c_int64), ("shadow_rays", C.c_int64), ("pieces", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self):
        return {"light_samples": int(self.light_samples), "shadow_rays": int(self.shadow_rays), "pieces": int(self.pieces)}


class DirectOpts(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("n_samples", C.c_int32), ("key_sample", C.c_uint32), ("reserved", C.c_int32 * 5)]


DIRECT_MAX_SAMPLES = 4096  # light samples per point of mcpt_query_direct
DIRECT_STREAM = 5          # the Philox stream of its light samples
PROBE_DEPTH_RES = 8  # MCPT_PROBE_DEPTH_RES
PROBE_DEPTH_ROW = PROBE_DEPTH_RES * PROBE_DEPTH_RES * 3  # floats of moments per probe


def _probe_depth_params(who, spp, max_distance, seed=1, sample_offset=0, accumulate=0):
    """mcpt_probe_depth_params; the library's refusals that depend on the parameters alone are made here as well."""
    spp, sample_offset, accumulate = int(spp), int(sample_offset), int(bool(accumulate))
    if spp <= 0 or sample_offset < 0 or sample_offset + spp > 2 ** 31 - 1:
        raise ValueError("%s: spp is positive, sample_offset >= 0 and sample_offset + spp at most 2^31 - 1, not %d and %d" % (who, spp, sample_offset))
    md = np.float32(max_distance)
    if not (md > 0 and np.isfinite(md)):
        raise ValueError("%s: max_distance is positive and finite, not %r" % (who, max_distance))
    return ProbeDepthParams(int(seed) & 0xffffffff, spp, sample_offset, accumulate, float(md), (C.c_int32 * 3)(0, 0, 0))


def _probe_visibility(who, normal_bias, backface_max):
    nb, bm = np.float32(normal_bias), np.float32(backface_max)
    if not (nb >= 0 and np.isfinite(nb) and bm >= 0 and np.isfinite(bm)):
        raise ValueError("%s: normal_bias and backface_max are finite and not negative, not %r and %r" % (who, normal_bias, backface_max))
    return ProbeVisibility(float(nb), float(bm), (C.c_int32 * 2)(0, 0))


class LitOpts(C.Structure):
    _fields_ = [("aov_spp", C.c_int32), ("specular_depth", C.c_int32), ("centre", C.c_int32), ("seed", C.c_uint32), ("reserved", C.c_int32 * 4)]


class ProbeVolume(C.Structure):
    _fields_ = [("grid", C.POINTER(ProbeGrid)), ("sh", C.c_void_p), ("moments", C.c_void_p), ("counts", C.c_void_p),
                ("visibility", C.POINTER(ProbeVisibility))]


class LitOutputs(C.Structure):
    _fields_ = [("lit", C.c_void_p), ("position", C.c_void_p), ("reserved", C.c_void_p * 2)]


class LitInfo(C.Structure):
    _fields_ = [("chunks", C.c_int32), ("in_workspace", C.c_int32), ("samples", C.c_int64), ("lookups", C.c_int64), ("ms_total", C.c_double)]

    def as_dict(self):
        return {"chunks": int(self.chunks), "in_workspace": int(self.in_workspace), "samples": int(self.samples), "lookups": int(self.lookups),
                "ms_total": float(self.ms_total)}


class ProbeRelightOpts(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("spp", C.c_int32), ("sample_offset", C.c_int32), ("hysteresis", C.c_float), ("indirect_only", C.c_int32),
                ("direct_samples", C.c_int32), ("direct_seed", C.c_uint32), ("max_distance", C.c_float), ("reserved", C.c_int32 * 8)]


class ProbeRelightOutputs(C.Structure):
    _fields_ = [("sh", C.c_void_p), ("moments", C.c_void_p), ("counts", C.c_void_p), ("reserved", C.c_void_p)]


def _probe_relight_opts(who, spp, seed, sample_offset, hysteresis, indirect_only, direct_samples, direct_seed, depth, max_distance):
    """mcpt_probe_relight_opts; the library's refusals that depend on the options alone are made here as well."""
    spp, sample_offset, direct_samples = int(spp), int(sample_offset), int(direct_samples)
    if spp < 1 or sample_offset < 0 or sample_offset + spp > 2 ** 31 - 1:
        raise ValueError("%s: spp is positive, sample_offset >= 0 and sample_offset + spp at most 2^31 - 1, not %d and %d" % (who, spp, sample_offset))
    h = np.float32(hysteresis)
    if not (h >= 0 and h < 1):
        raise ValueError("%s: hysteresis is in [0, 1) as a float32, not %r" % (who, hysteresis))
    if not 0 <= direct_samples <= DIRECT_MAX_SAMPLES:
        raise ValueError("%s: direct_samples must be in 0 .. %d, not %r" % (who, DIRECT_MAX_SAMPLES, direct_samples))
    md = np.float32(0.0 if max_distance is None else max_distance)
    if depth and not (md > 0 and np.isfinite(md)):
        raise ValueError("%s: max_distance is positive and finite when depth is asked, not %r" % (who, max_distance))
    return ProbeRelightOpts(int(seed) & 0xffffffff, spp, sample_offset, float(h), int(bool(indirect_only)), direct_samples, int(direct_seed) & 0xffffffff,
                            float(md), (C.c_int32 * 8)(*([0] * 8)))


def _lit_opts(who, aov_spp, specular_depth, centre, seed):
    """mcpt_lit_opts; the library's refusals that depend on the options alone are made here as well."""
    aov_spp, specular_depth, centre = int(aov_spp), int(specular_depth), int(bool(centre))
    if not 0 <= aov_spp <= 65536 or not 0 <= specular_depth <= 8:
        raise ValueError("%s: aov_spp is 0..65536 and specular_depth 0..8, not %d and %d" % (who, aov_spp, specular_depth))
    if centre and aov_spp > 1:
        raise ValueError("%s: centre takes one ray per pixel (aov_spp 0 or 1), not %d" % (who, aov_spp))
    return LitOpts(aov_spp, specular_depth, centre, int(seed) & 0xffffffff, (C.c_int32 * 4)(0, 0, 0, 0))


def _vertex_items(items, n_tri_of):
    """An iterable of (object index, vertices) as an array of mcpt_object_vertices.  n_tri_of: the triangle count of each mesh object, -1
    for the objects the library refuses anyway; `keep` holds the host arrays for the duration of the call."""
    items = list(items)
    arr, keep = (ObjectVertices * max(len(items), 1))(), []
    for k, (obj, v) in enumerate(items):
        obj = int(obj)
        dev = _device_positions(v)
        if dev is not None:
            n_tri, ptr, on_device = dev.n_tri, dev.ptr, 1
        else:
            if not isinstance(v, np.ndarray) or v.dtype != np.float32 or not v.flags["C_CONTIGUOUS"]:
                raise ValueError("deform: vertices are a C-contiguous float32 array, a device buffer or DevicePositions")
            if not ((v.ndim == 3 and v.shape[1:] == (3, 3)) or v.ndim == 1) or v.size % 9:
                raise ValueError("deform: positions have shape (n_tri, 3, 3) or (n_tri * 9,), not %s" % (v.shape,))
            keep.append(v)
            n_tri, ptr, on_device = v.size // 9, (v.ctypes.data if v.size else C.addressof(arr)), 0
        if 0 <= obj < len(n_tri_of) and n_tri_of[obj] >= 0 and n_tri != int(n_tri_of[obj]):
            raise ValueError("deform: object %d has %d triangles, the positions given describe %d" % (obj, int(n_tri_of[obj]), n_tri))
        arr[k].object, arr[k].on_device, arr[k].positions = obj, on_device, ptr
    return arr, len(items), keep


def _mesh_tri_counts(sd):
    """Per object: its triangle count (-1 for a sphere, which the library refuses)."""
    o = sd.objects
    return np.where(o["kind"] == 0, o["n_tri"], -1)


def _moves(moves):
    """An iterable of (object index, 3x4 array) as an array of mcpt_object_transform."""
    moves = list(moves)
    arr = (ObjectTransform * max(len(moves), 1))()
    for k, (obj, m) in enumerate(moves):
        m = np.asarray(m, dtype=np.float32)
        if m.shape != (3, 4):
            raise ValueError("a transform is a 3x4 array, not %s" % (m.shape,))
        arr[k].object = int(obj)
        arr[k].m = (C.c_float * 12)(*[float(x) for x in m.reshape(-1)])
    return arr, len(moves)


_libs = {}


def lib(path=None):
    """Loads libmcpt_hip.so (or the library at `path`); raises if it has not been built (run __graft_entry__.build())."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise FileNotFoundError("%s is missing: build it with `python __graft_entry__.py` (hipcc, gfx950)" % path)
        L = C.CDLL(path)
        L.mcpt_last_error.restype = C.c_char_p
        L.mcpt_version.restype = C.c_char_p
        L.mcpt_scene_create.restype = C.c_int
        L.mcpt_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.mcpt_scene_create_ex.restype = C.c_int
        L.mcpt_scene_create_ex.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mcpt_scene_dump_bvh.restype = C.c_int
        L.mcpt_scene_dump_bvh.argtypes = [C.c_void_p, C.POINTER(BvhInfo), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_tonemap.restype = C.c_int
        L.mcpt_tonemap.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        L.mcpt_tonemap_device.restype = C.c_int
        L.mcpt_tonemap_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mcpt_scene_destroy.restype = None
        L.mcpt_scene_destroy.argtypes = [C.c_void_p]
        L.mcpt_scene_get_info.restype = C.c_int
        L.mcpt_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
        L.mcpt_scene_ray_counts.restype = C.c_int
        L.mcpt_scene_ray_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcpt_scene_primary_conductor_counts.restype = C.c_int
        L.mcpt_scene_primary_conductor_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.mcpt_bvh_dump.restype = C.c_int
        L.mcpt_bvh_dump.argtypes = [C.POINTER(SceneDesc), C.POINTER(BvhInfo), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_render.restype = C.c_int
        L.mcpt_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(Stats)]
        L.mcpt_render_adaptive.restype = C.c_int
        L.mcpt_render_adaptive.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Adaptive), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(AdaptiveInfo), C.POINTER(Stats)]
        L.mcpt_render_aovs.restype = C.c_int
        L.mcpt_render_aovs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        L.mcpt_render_aovs_ex.restype = C.c_int
        L.mcpt_render_aovs_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p]
        L.mcpt_denoise.restype = C.c_int
        L.mcpt_denoise.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseOpts), C.c_void_p]
        L.mcpt_render_denoised.restype = C.c_int
        L.mcpt_render_denoised.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(DenoiseOpts), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.POINTER(DenoiseInfo), C.POINTER(Stats)]
        L.mcpt_scene_snapshot.restype = C.c_int
        L.mcpt_scene_snapshot.argtypes = [C.c_void_p]
        L.mcpt_render_motion.restype = C.c_int
        L.mcpt_render_motion.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p]
        L.mcpt_render_motion_ex.restype = C.c_int
        L.mcpt_render_motion_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_void_p]
        L.mcpt_sequence_create_motion.restype = C.c_int
        L.mcpt_sequence_create_motion.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                  C.POINTER(SequenceAdaptive), C.POINTER(SequenceMotion), C.POINTER(C.c_void_p)]
        L.mcpt_temporal_blend.restype = C.c_int
        L.mcpt_temporal_blend.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.POINTER(TemporalOpts), C.c_void_p, C.c_void_p]
        L.mcpt_temporal_accumulate.restype = C.c_int
        L.mcpt_temporal_accumulate.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7 + [C.POINTER(TemporalOpts)] + [C.c_void_p] * 3
        L.mcpt_temporal_accumulate_ex.restype = C.c_int
        L.mcpt_temporal_accumulate_ex.argtypes = ([C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 9 + [C.POINTER(TemporalOpts), C.POINTER(HistoryOpts)]
                                                  + [C.c_void_p] * 4)
        L.mcpt_temporal_accumulate_weighted.restype = C.c_int
        L.mcpt_temporal_accumulate_weighted.argtypes = ([C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5 + [C.c_float] + [C.c_void_p] * 6
                                                        + [C.POINTER(TemporalOpts), C.POINTER(HistoryOpts)] + [C.c_void_p] * 5)
        L.mcpt_temporal_history_weight.restype = C.c_int
        L.mcpt_temporal_history_weight.argtypes = ([C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 7
                                                   + [C.POINTER(TemporalOpts), C.POINTER(HistoryOpts), C.c_void_p])
        L.mcpt_render_adaptive_weighted.restype = C.c_int
        L.mcpt_render_adaptive_weighted.argtypes = ([C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Adaptive), C.c_void_p, C.c_int32]
                                                    + [C.c_void_p] * 4 + [C.POINTER(AdaptiveInfo), C.POINTER(Stats)])
        L.mcpt_sequence_create_weighted.restype = C.c_int
        L.mcpt_sequence_create_weighted.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                    C.POINTER(SequenceAdaptive), C.POINTER(SequenceMotion), C.POINTER(SequenceWeighted),
                                                    C.POINTER(C.c_void_p)]
        L.mcpt_sequence_weight.restype = C.c_int
        L.mcpt_sequence_weight.argtypes = [C.c_void_p, C.c_void_p]
        L.mcpt_temporal_accumulate_moments.restype = C.c_int
        L.mcpt_temporal_accumulate_moments.argtypes = ([C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 8
                                                       + [C.POINTER(TemporalOpts), C.POINTER(HistoryOpts)] + [C.c_void_p] * 4)
        L.mcpt_moments_variance.restype = C.c_int
        L.mcpt_moments_variance.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(MomentsOpts), C.c_void_p]
        L.mcpt_sequence_create_moments.restype = C.c_int
        L.mcpt_sequence_create_moments.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                   C.POINTER(SequenceAdaptive), C.POINTER(SequenceMotion), C.POINTER(SequenceWeighted),
                                                   C.POINTER(MomentsOpts), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_create_features.restype = C.c_int
        L.mcpt_sequence_create_features.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                    C.POINTER(SequenceAdaptive), C.POINTER(SequenceMotion), C.POINTER(SequenceWeighted),
                                                    C.POINTER(MomentsOpts), C.POINTER(FeatureOpts), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_create_feedback.restype = C.c_int
        L.mcpt_sequence_create_feedback.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                    C.POINTER(SequenceAdaptive), C.POINTER(SequenceMotion), C.POINTER(SequenceWeighted),
                                                    C.POINTER(MomentsOpts), C.POINTER(FeatureOpts), C.POINTER(FeedbackOpts), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_history.restype = C.c_int
        L.mcpt_sequence_history.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_denoise_feedback.restype = C.c_int
        L.mcpt_denoise_feedback.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(DenoiseOpts),
                                            C.POINTER(FeedbackOpts), C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_centre_rays.restype = C.c_int
        L.mcpt_centre_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3
        L.mcpt_render_aovs_features.restype = C.c_int
        L.mcpt_render_aovs_features.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(FeatureOpts), C.c_void_p]
        L.mcpt_render_motion_features.restype = C.c_int
        L.mcpt_render_motion_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.POINTER(FeatureOpts),
                                                  C.c_void_p]
        L.mcpt_sequence_moments.restype = C.c_int
        L.mcpt_sequence_moments.argtypes = [C.c_void_p, C.c_void_p]
        L.mcpt_sequence_create_ex.restype = C.c_int
        L.mcpt_sequence_create_ex.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_flags.restype = C.c_int
        L.mcpt_sequence_flags.argtypes = [C.c_void_p, C.c_void_p]
        L.mcpt_temporal_history_len.restype = C.c_int
        L.mcpt_temporal_history_len.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 6 + [C.POINTER(TemporalOpts), C.POINTER(HistoryOpts), C.c_void_p]
        L.mcpt_render_adaptive_guided.restype = C.c_int
        L.mcpt_render_adaptive_guided.argtypes = ([C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Adaptive)] + [C.c_void_p] * 5
                                                  + [C.POINTER(AdaptiveInfo), C.POINTER(Stats)])
        L.mcpt_render_adaptive_denoised.restype = C.c_int
        L.mcpt_render_adaptive_denoised.argtypes = ([C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(Adaptive), C.c_void_p, C.POINTER(DenoiseOpts)]
                                                    + [C.c_void_p] * 6 + [C.POINTER(AdaptiveInfo), C.POINTER(DenoiseInfo), C.POINTER(Stats)])
        L.mcpt_sequence_create_adaptive.restype = C.c_int
        L.mcpt_sequence_create_adaptive.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(HistoryOpts),
                                                    C.POINTER(SequenceAdaptive), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_counts.restype = C.c_int
        L.mcpt_sequence_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveInfo)]
        L.mcpt_sequence_create.restype = C.c_int
        L.mcpt_sequence_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(SequenceOpts), C.POINTER(C.c_void_p)]
        L.mcpt_sequence_frame.restype = C.c_int
        L.mcpt_sequence_frame.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.POINTER(SequenceOutputs), C.POINTER(SequenceInfo), C.POINTER(Stats)]
        L.mcpt_sequence_reset.restype = C.c_int
        L.mcpt_sequence_reset.argtypes = [C.c_void_p]
        L.mcpt_sequence_destroy.restype = None
        L.mcpt_sequence_destroy.argtypes = [C.c_void_p]
        L.mcpt_render_device.restype = C.c_int
        L.mcpt_render_device.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mcpt_intersect.restype = C.c_int
        L.mcpt_intersect.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_query_closest.restype = C.c_int
        L.mcpt_query_closest.argtypes = [C.c_void_p, C.c_int64, C.POINTER(RayBuffers), C.POINTER(HitBuffers), C.c_void_p, C.POINTER(QueryInfo)]
        L.mcpt_query_occluded.restype = C.c_int
        L.mcpt_query_occluded.argtypes = [C.c_void_p, C.c_int64, C.POINTER(RayBuffers), C.c_void_p, C.c_void_p, C.POINTER(QueryInfo)]
        L.mcpt_query_radiance.restype = C.c_int
        L.mcpt_query_radiance.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int64, C.POINTER(SensorBuffers), C.POINTER(SensorOutputs), C.c_void_p, C.POINTER(Stats)]
        L.mcpt_sensor_rays.restype = C.c_int
        L.mcpt_sensor_rays.argtypes = [C.c_void_p, C.c_int32, C.c_uint32, C.c_int64] + [C.c_void_p] * 6
        L.mcpt_query_probes.restype = C.c_int
        L.mcpt_query_probes.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int64, C.c_void_p, C.POINTER(ProbeOutputs), C.c_void_p, C.POINTER(Stats)]
        L.mcpt_probe_rays.restype = C.c_int
        L.mcpt_probe_rays.argtypes = [C.c_void_p, C.c_uint32, C.c_int64] + [C.c_void_p] * 5
        L.mcpt_probe_shade.restype = C.c_int
        L.mcpt_probe_shade.argtypes = [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_bake_probe_grid.restype = C.c_int
        L.mcpt_bake_probe_grid.argtypes = [C.c_void_p, C.POINTER(ProbeGrid), C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.mcpt_scene_probe_buffers.restype = C.c_int
        L.mcpt_scene_probe_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mcpt_sh_basis_host.restype = C.c_int
        L.mcpt_sh_basis_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        L.mcpt_sh_irradiance_host.restype = C.c_int
        L.mcpt_sh_irradiance_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_probe_grid_points_host.restype = C.c_int
        L.mcpt_probe_grid_points_host.argtypes = [C.POINTER(ProbeGrid), C.c_void_p]
        L.mcpt_probe_shade_host.restype = C.c_int
        L.mcpt_probe_shade_host.argtypes = [C.POINTER(ProbeGrid), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_query_probe_depth.restype = C.c_int
        L.mcpt_query_probe_depth.argtypes = [C.c_void_p, C.POINTER(ProbeDepthParams), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(QueryInfo)]
        L.mcpt_probe_shade_visible.restype = C.c_int
        L.mcpt_probe_shade_visible.argtypes = [C.c_void_p, C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProbeVisibility), C.c_int64] + [C.c_void_p] * 5
        L.mcpt_bake_probe_volume.restype = C.c_int
        L.mcpt_bake_probe_volume.argtypes = [C.c_void_p, C.POINTER(ProbeGrid), C.POINTER(Params), C.POINTER(ProbeDepthParams)] + [C.c_void_p] * 4 + [C.POINTER(Stats)]
        L.mcpt_query_probes_ex.restype = C.c_int
        L.mcpt_query_probes_ex.argtypes = list(L.mcpt_query_probes.argtypes) + [C.POINTER(ProbeOpts)]
        L.mcpt_bake_probe_grid_ex.restype = C.c_int
        L.mcpt_bake_probe_grid_ex.argtypes = list(L.mcpt_bake_probe_grid.argtypes) + [C.POINTER(ProbeOpts)]
        L.mcpt_bake_probe_volume_ex.restype = C.c_int
        L.mcpt_bake_probe_volume_ex.argtypes = list(L.mcpt_bake_probe_volume.argtypes) + [C.POINTER(ProbeOpts)]
        L.mcpt_render_probe_lit_direct.restype = C.c_int
        L.mcpt_render_probe_lit_direct.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LitOpts), C.POINTER(LitDirectOpts), C.POINTER(ProbeVolume), C.POINTER(LitOutputs),
                                                   C.c_void_p, C.POINTER(LitInfo), C.POINTER(LitDirectInfo)]
        L.mcpt_probe_volume_relight.restype = C.c_int
        L.mcpt_probe_volume_relight.argtypes = [C.c_void_p, C.POINTER(ProbeVolume), C.POINTER(ProbeRelightOpts), C.POINTER(ProbeRelightOutputs), C.c_void_p,
                                                C.POINTER(QueryInfo)]
        L.mcpt_probe_relight_fold_host.restype = C.c_int
        L.mcpt_probe_relight_fold_host.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.mcpt_query_direct.restype = C.c_int
        L.mcpt_query_direct.argtypes = [C.c_void_p, C.POINTER(DirectOpts), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(QueryInfo)]
        L.mcpt_rng_uniforms_host.restype = C.c_int
        L.mcpt_rng_uniforms_host.argtypes = [C.c_uint32, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_direct_samples_host.restype = C.c_int
        L.mcpt_direct_samples_host.argtypes = [C.c_int64, C.c_int32] + [C.c_void_p] * 8
        L.mcpt_direct_fold_host.restype = C.c_int
        L.mcpt_direct_fold_host.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_probe_depth_dirs_host.restype = C.c_int
        L.mcpt_probe_depth_dirs_host.argtypes = [C.c_void_p]
        L.mcpt_probe_depth_texel_host.restype = C.c_int
        L.mcpt_probe_depth_texel_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
        L.mcpt_probe_depth_fold_host.restype = C.c_int
        L.mcpt_probe_depth_fold_host.argtypes = [C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.mcpt_render_probe_lit.restype = C.c_int
        L.mcpt_render_probe_lit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(LitOpts), C.POINTER(ProbeVolume), C.POINTER(LitOutputs), C.c_void_p, C.POINTER(LitInfo)]
        L.mcpt_probe_shade_visible_host.restype = C.c_int
        L.mcpt_probe_shade_visible_host.argtypes = [C.POINTER(ProbeGrid), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(ProbeVisibility), C.c_int64] + [C.c_void_p] * 4
        L.mcpt_lightmap_texels.restype = C.c_int
        L.mcpt_lightmap_texels.argtypes = [C.c_void_p, C.POINTER(LightmapDesc), C.POINTER(LightmapTexelsOut), C.POINTER(C.c_int64), C.c_void_p]
        L.mcpt_lightmap_scatter.restype = C.c_int
        L.mcpt_lightmap_scatter.argtypes = [C.c_void_p, C.POINTER(LightmapDesc), C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_bake_lightmap.restype = C.c_int
        L.mcpt_bake_lightmap.argtypes = [C.c_void_p, C.POINTER(LightmapDesc), C.POINTER(Params), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(LightmapInfo), C.POINTER(Stats)]
        L.mcpt_lightmap_texels_host.restype = C.c_int
        L.mcpt_lightmap_texels_host.argtypes = [C.POINTER(SceneDesc), C.POINTER(LightmapDesc)] + [C.c_void_p] * 5 + [C.POINTER(C.c_int64)]
        L.mcpt_lightmap_dilate_host.restype = C.c_int
        L.mcpt_lightmap_dilate_host.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.mcpt_cast_rays.restype = C.c_int
        L.mcpt_cast_rays.argtypes = [C.c_void_p, C.POINTER(Params), C.c_int64] + [C.c_void_p] * 6
        L.mcpt_camera_rays.restype = C.c_int
        L.mcpt_camera_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64] + [C.c_void_p] * 4
        L.mcpt_debug_fmath.restype = C.c_int
        L.mcpt_debug_fmath.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_debug_scene.restype = C.c_int
        L.mcpt_debug_scene.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]
        L.mcpt_debug_shadow.restype = C.c_int
        L.mcpt_debug_shadow.argtypes = [C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 6
        L.mcpt_debug_material.restype = C.c_int
        L.mcpt_debug_material.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_scene_update.restype = C.c_int
        L.mcpt_scene_update.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(UpdateInfo)]
        L.mcpt_group_update.restype = C.c_int
        L.mcpt_group_update.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.mcpt_transform_triangles.restype = C.c_int
        L.mcpt_transform_triangles.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.mcpt_scene_deform.restype = C.c_int
        L.mcpt_scene_deform.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(UpdateInfo)]
        L.mcpt_group_deform.restype = C.c_int
        L.mcpt_group_deform.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.mcpt_scene_set_materials.restype = C.c_int
        L.mcpt_scene_set_materials.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(UpdateInfo)]
        L.mcpt_scene_set_environment.restype = C.c_int
        L.mcpt_scene_set_environment.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(UpdateInfo)]
        L.mcpt_group_set_materials.restype = C.c_int
        L.mcpt_group_set_materials.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
        L.mcpt_group_set_environment.restype = C.c_int
        L.mcpt_group_set_environment.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
        L.mcpt_scene_set_visibility.restype = C.c_int
        L.mcpt_scene_set_visibility.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(UpdateInfo)]
        L.mcpt_scene_get_visibility.restype = C.c_int
        L.mcpt_scene_get_visibility.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32)]
        L.mcpt_group_set_visibility.restype = C.c_int
        L.mcpt_group_set_visibility.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        L.mcpt_compact_scene.restype = C.c_int
        L.mcpt_compact_scene.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        L.mcpt_scene_add_objects.restype = C.c_int
        L.mcpt_scene_add_objects.argtypes = [C.c_void_p, C.POINTER(SceneAddition), C.POINTER(C.c_int32), C.POINTER(UpdateInfo)]
        L.mcpt_group_add_objects.restype = C.c_int
        L.mcpt_group_add_objects.argtypes = [C.c_void_p, C.POINTER(SceneAddition), C.POINTER(C.c_int32)]
        L.mcpt_extend_scene.restype = C.c_int
        L.mcpt_extend_scene.argtypes = [C.c_void_p, C.POINTER(SceneAddition), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32)]
        L.mcpt_deform_triangles.restype = C.c_int
        L.mcpt_deform_triangles.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcpt_group_create.restype = C.c_int
        L.mcpt_group_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.mcpt_group_render.restype = C.c_int
        L.mcpt_group_render.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_void_p, C.POINTER(Stats)]
        L.mcpt_group_get_info.restype = C.c_int
        L.mcpt_group_get_info.argtypes = [C.c_void_p, C.POINTER(GroupInfo)]
        L.mcpt_group_scene.restype = C.c_void_p
        L.mcpt_group_scene.argtypes = [C.c_void_p, C.c_int]
        L.mcpt_group_size.restype = C.c_int
        L.mcpt_group_size.argtypes = [C.c_void_p]
        L.mcpt_group_destroy.restype = None
        L.mcpt_group_destroy.argtypes = [C.c_void_p]
        L.mcpt_group_last_error.restype = C.c_char_p
        L.mcpt_debug_counters.restype = C.c_int
        L.mcpt_debug_counters.argtypes = [C.c_void_p, C.c_void_p]
        L.mcpt_cull_bound.restype = C.c_int
        L.mcpt_cull_bound.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CullInfo)]
        L.mcpt_debug_classify.restype = C.c_int
        L.mcpt_debug_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CullInfo)]
        _libs[path] = L
    return _libs[path]


def _check(rc, allow=(), L=None):
    if rc != 0 and rc not in allow:
        raise McptError(rc, (L or lib()).mcpt_last_error().decode("utf-8", "replace"))
    return rc


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class BvhInfo(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("root", C.c_int32), ("stack_entries", C.c_int32), ("quantised", C.c_int32),
                ("root_min", C.c_float * 3), ("root_max", C.c_float * 3), ("q_origin", C.c_float * 3), ("q_cell", C.c_float * 3),
                ("n_instances", C.c_int32), ("n_leaf_prims", C.c_int32)]


def _make_desc(sd, keep):
    """SceneDesc over the arrays of a scenes.SceneData; `keep` receives the arrays that must outlive the call."""
    tri, mat, obj = np.ascontiguousarray(sd.triangles), np.ascontiguousarray(sd.materials), np.ascontiguousarray(sd.objects)
    keep.extend([tri, mat, obj])
    d = SceneDesc()
    d.n_objects, d.n_triangles, d.n_materials = len(obj), len(tri), len(mat)
    d.background = (C.c_float * 3)(*[float(x) for x in sd.background])
    d.objects, d.triangles, d.materials = _ptr(obj), _ptr(tri), _ptr(mat)
    if sd.env_pixels is not None:
        env = np.ascontiguousarray(sd.env_pixels, dtype=np.float32)
        keep.append(env)
        d.env_h, d.env_w = env.shape[:2]
        d.env_pixels = _ptr(env)
    return d


def transform_triangles(m, tris, out=None):
    """mcpt_transform_triangles (host only): the triangles (scenes.TRI_DTYPE) with every vertex moved by the row-major 3x4 matrix m under the
    rule of mcpt_scene_update; the texture coordinates are copied.  out: the array to write (may be `tris` itself); default a new one."""
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    if m.size != 12:
        raise ValueError("a transform is a 3x4 array")
    if not tris.flags["C_CONTIGUOUS"]:
        tris = np.ascontiguousarray(tris)
    if out is None:
        out = np.empty_like(tris)
    if out.dtype != tris.dtype or out.shape != tris.shape or not out.flags["C_CONTIGUOUS"] or tris.dtype.itemsize != 60:
        raise ValueError("transform_triangles: arrays of 60-byte triangles with one shape")
    _check(lib().mcpt_transform_triangles(_ptr(m), tris.size, _ptr(tris), _ptr(out)))
    return out


def deform_triangles(positions, tris, out=None):
    """mcpt_deform_triangles (host only): the triangles (scenes.TRI_DTYPE) with their vertices replaced by `positions`, a C-contiguous float32
    array of shape (n_tri, 3, 3) or (n_tri * 9,); the texture coordinates are copied.  out: the array to write (may be `tris` itself)."""
    if not isinstance(positions, np.ndarray) or positions.dtype != np.float32 or not positions.flags["C_CONTIGUOUS"]:
        raise ValueError("deform_triangles: positions are a C-contiguous float32 array")
    if not tris.flags["C_CONTIGUOUS"]:
        tris = np.ascontiguousarray(tris)
    if positions.size != tris.size * 9:
        raise ValueError("deform_triangles: %d triangles need %d position floats, not %d" % (tris.size, tris.size * 9, positions.size))
    if out is None:
        out = np.empty_like(tris)
    if out.dtype != tris.dtype or out.shape != tris.shape or not out.flags["C_CONTIGUOUS"] or tris.dtype.itemsize != 60:
        raise ValueError("deform_triangles: arrays of 60-byte triangles with one shape")
    _check(lib().mcpt_deform_triangles(tris.size, _ptr(positions), _ptr(tris), _ptr(out)))
    return out


def compact_scene(sd, visible):
    """mcpt_compact_scene (host only): the description without the objects whose entry of `visible` (one per object) is false.  Returns
    (SceneData, prim_map): prim_map[p] is the id that primitive p of `sd` has in the result, -1 if it is hidden."""
    import dataclasses
    vis = np.ascontiguousarray(np.asarray(visible).astype(bool), dtype=np.uint8)
    if vis.shape != (len(sd.objects),):
        raise ValueError("compact_scene: one flag per object (%d), not %s" % (len(sd.objects), vis.shape))
    keep = []
    d = _make_desc(sd, keep)
    no, nt = C.c_int32(0), C.c_int32(0)
    prim_map = np.full(len(sd.triangles) + len(sd.objects), -1, np.int32)
    _check(lib().mcpt_compact_scene(C.byref(d), _ptr(vis), None, None, C.byref(no), C.byref(nt), _ptr(prim_map)))
    objects, triangles = np.zeros(no.value, sd.objects.dtype), np.zeros(nt.value, sd.triangles.dtype)
    _check(lib().mcpt_compact_scene(C.byref(d), _ptr(vis), _ptr(objects), _ptr(triangles), C.byref(no), C.byref(nt), _ptr(prim_map)))
    return dataclasses.replace(sd, objects=objects, triangles=triangles), prim_map


def extend_scene(sd, objects, triangles, materials=None):
    """mcpt_extend_scene (host only): the description `sd` followed by the given objects (records of sd.objects' dtype; first_tri relative
    to `triangles`, material an index into the table after the append), their triangles and the given materials.  Returns the SceneData."""
    import dataclasses
    keep = []
    d = _make_desc(sd, keep)
    a, arrays = _addition(sd, objects, triangles, materials)
    no, nt, nm = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().mcpt_extend_scene(C.byref(d), C.byref(a), None, None, None, C.byref(no), C.byref(nt), C.byref(nm)))
    obj, tri, mat = np.zeros(no.value, sd.objects.dtype), np.zeros(nt.value, sd.triangles.dtype), np.zeros(nm.value, sd.materials.dtype)
    _check(lib().mcpt_extend_scene(C.byref(d), C.byref(a), _ptr(obj), _ptr(tri), _ptr(mat), C.byref(no), C.byref(nt), C.byref(nm)))
    del arrays
    return dataclasses.replace(sd, objects=obj, triangles=tri, materials=mat)


def lightmap_texels(sd, object, width, height, flip_normals=False):
    """mcpt_lightmap_texels_host (host only): the texel sensors of one mesh object of a description under the rule of include/mcpt.h ->
    dict of numpy arrays texel (n,), prim (n,), bary (n, 2), origins (n, 3), normals (n, 3), in ascending texel order."""
    keep = []
    d = _make_desc(sd, keep)
    ld = _lightmap_desc(object, width, height, flip_normals)
    cap = max(int(width), 0) * max(int(height), 0)
    if cap > (2 ** 31 - 1) // 3:
        cap = 0  # (the library refuses the size before it writes anything)
    out = {w: np.zeros(_row_shape(cap, k), dt) for w, (dt, k) in LIGHTMAP_OUTPUTS.items()}
    n = C.c_int64(0)
    _check(lib().mcpt_lightmap_texels_host(C.byref(d), C.byref(ld), *[_ptr(out[w]) for w in LIGHTMAP_OUTPUTS], C.byref(n)))
    return {w: out[w][:n.value].copy() for w in LIGHTMAP_OUTPUTS}


def lightmap_dilate(width, height, texel, values, dilate):
    """mcpt_lightmap_dilate_host (host only): scatter `values` (n, 3) to the listed texels of a zero map and run `dilate` rounds of the
    dilation of include/mcpt.h -> (image (height, width, 3) float32, coverage (height, width) uint8: 0 empty, 1 scattered, 2 dilated)."""
    tx = np.ascontiguousarray(texel, dtype=np.int32).reshape(-1)
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 3)
    if len(v) != len(tx):
        raise ValueError("lightmap_dilate: one value row per texel")
    W, H = int(width), int(height)
    big = W < 1 or H < 1 or W * H > (2 ** 31 - 1) // 3
    image = np.zeros((1, 1, 3) if big else (H, W, 3), np.float32)
    cov = np.zeros((1, 1) if big else (H, W), np.uint8)
    _check(lib().mcpt_lightmap_dilate_host(W, H, len(tx), _ptr(tx), _ptr(v), int(dilate), _ptr(image), _ptr(cov)))
    return image, cov


def sh_basis(dirs):
    """mcpt_sh_basis_host (host only): the nine real spherical harmonics of order <= 2 at unit directions (n, 3) -> (n, 9) float32, in the
    index order of include/mcpt.h."""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((len(d), 9), np.float32)
    _check(lib().mcpt_sh_basis_host(len(d), _ptr(d), _ptr(out)))
    return out


def sh_irradiance(sh, normals):
    """mcpt_sh_irradiance_host (host only): E / pi for unit normals (n, 3) from coefficients (n, 27), or (27,) for all of them -> (n, 3)
    float32.  Not clamped at zero."""
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    L = np.ascontiguousarray(sh, dtype=np.float32)
    if L.size == 27:
        L = np.ascontiguousarray(np.broadcast_to(L.reshape(1, 27), (len(nr), 27)))
    if L.shape != (len(nr), 27):
        raise ValueError("sh_irradiance: sh has shape (27,) or (n, 27), not %s" % (L.shape,))
    out = np.zeros((len(nr), 3), np.float32)
    _check(lib().mcpt_sh_irradiance_host(len(nr), _ptr(L), _ptr(nr), _ptr(out)))
    return out


def probe_grid_points(origin, spacing, dims):
    """mcpt_probe_grid_points_host (host only): the points of a probe grid -> (nx*ny*nz, 3) float32, probe (ix, iy, iz) in row
    (iz * ny + iy) * nx + ix."""
    g, n = _probe_grid("probe_grid_points", origin, spacing, dims)
    out = np.zeros((n, 3), np.float32)
    _check(lib().mcpt_probe_grid_points_host(C.byref(g), _ptr(out)))
    return out


def probe_shade(origin, spacing, dims, sh, points, normals):
    """mcpt_probe_shade_host (host only): the trilinear grid lookup of include/mcpt.h, E / pi at `points` (n, 3) for `normals` (n, 3) from
    the grid's coefficients sh (probes, 27) -> (n, 3) float32."""
    g, m = _probe_grid("probe_shade", origin, spacing, dims)
    L = np.ascontiguousarray(sh, dtype=np.float32)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    if L.shape != (m, 27) or len(nr) != len(p):
        raise ValueError("probe_shade: sh has shape (%d, 27) and there is one normal per point, not %s, %d and %d" % (m, L.shape, len(nr), len(p)))
    out = np.zeros((len(p), 3), np.float32)
    _check(lib().mcpt_probe_shade_host(C.byref(g), _ptr(L), len(p), _ptr(p), _ptr(nr), _ptr(out)))
    return out


def rng_uniforms(seed, pixel, sample, depth, block, stream):
    """mcpt_rng_uniforms_host (host only): the Philox block of key (seed, pixel) and counter (sample, depth, block, stream) as four uniforms
    per row -> (n, 4) float32.  sample, depth, block and stream broadcast against each other."""
    a = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint32) for v in (sample, depth, block, stream)])
    a = [np.ascontiguousarray(v.reshape(-1)) for v in a]
    n = len(a[0])
    out = np.zeros((n, 4), dtype=np.float32)
    _check(lib().mcpt_rng_uniforms_host(int(seed) & 0xffffffff, int(pixel) & 0xffffffff, n, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), _ptr(out)))
    return out


def direct_samples(points, normals, light_rows):
    """mcpt_direct_samples_host (host only): the geometry of the sampled direct term of include/mcpt.h for points (n, 3), unit normals (n, 3)
    and light samples light_rows (n, N, 10: the rows of HipScene.sample_light) -> a dict of q (n, N, 3), ws (n, N, 3), dist (n, N), live
    (n, N) uint8 and contrib (n, N, 3) = emit * g / N."""
    p = np.ascontiguousarray(points, dtype=np.float32)
    nr = np.ascontiguousarray(normals, dtype=np.float32)
    r = np.ascontiguousarray(light_rows, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or nr.shape != p.shape:
        raise ValueError("direct_samples: points and normals have shape (n, 3), not %s and %s" % (p.shape, nr.shape))
    n = len(p)
    if r.ndim != 3 or r.shape[0] != n or r.shape[1] < 1 or r.shape[2] != 10:
        raise ValueError("direct_samples: light_rows has shape (%d, N, 10) with N >= 1, not %s" % (n, r.shape))
    N = r.shape[1]
    out = {"q": np.zeros((n, N, 3), np.float32), "ws": np.zeros((n, N, 3), np.float32), "dist": np.zeros((n, N), np.float32),
           "live": np.zeros((n, N), np.uint8), "contrib": np.zeros((n, N, 3), np.float32)}
    _check(lib().mcpt_direct_samples_host(n, N, _ptr(p), _ptr(nr), _ptr(r), _ptr(out["q"]), _ptr(out["ws"]), _ptr(out["dist"]), _ptr(out["live"]),
                                          _ptr(out["contrib"])))
    return out


def direct_fold(contrib, visible):
    """mcpt_direct_fold_host (host only): D of include/mcpt.h from the contributions (n, N, 3) and the visibility (n, N; non-zero: visible)
    of every light sample -> (n, 3) float32."""
    c = np.ascontiguousarray(contrib, dtype=np.float32)
    if c.ndim != 3 or c.shape[1] < 1 or c.shape[2] != 3:
        raise ValueError("direct_fold: contrib has shape (n, N, 3) with N >= 1, not %s" % (c.shape,))
    v = np.ascontiguousarray(np.asarray(visible) != 0, dtype=np.uint8)
    if v.shape != c.shape[:2]:
        raise ValueError("direct_fold: visible has shape %s, not %s" % (c.shape[:2], v.shape))
    out = np.zeros((c.shape[0], 3), dtype=np.float32)
    _check(lib().mcpt_direct_fold_host(c.shape[0], c.shape[1], _ptr(c), _ptr(v), _ptr(out)))
    return out


def probe_depth_dirs():
    """mcpt_probe_depth_dirs_host (host only): the unit directions of the 64 texels of a probe's depth map -> (64, 3) float32."""
    out = np.zeros((PROBE_DEPTH_RES * PROBE_DEPTH_RES, 3), np.float32)
    _check(lib().mcpt_probe_depth_dirs_host(_ptr(out)))
    return out


def probe_depth_texel(v):
    """mcpt_probe_depth_texel_host (host only): the nearest depth-map texel of vectors (n, 3) -> (n,) int32."""
    v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(v), np.int32)
    _check(lib().mcpt_probe_depth_texel_host(len(v), _ptr(v), _ptr(out)))
    return out


def probe_depth_fold(dirs, r, backfacing, moments=None, counts=None):
    """mcpt_probe_depth_fold_host (host only): the fold of include/mcpt.h over given samples -- dirs (n, spp, 3), r (n, spp), backfacing
    (n, spp) -> (moments (n, 192) float32, counts (n, 2) int32).  With moments and counts (both or neither) the fold continues them
    (accumulate = 1); the inputs are not changed."""
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 3 or d.shape[1] < 1:
        raise ValueError("probe_depth_fold: dirs has shape (n, spp, 3) with spp >= 1, not %s" % (d.shape,))
    n, spp = d.shape[0], d.shape[1]
    rr = np.ascontiguousarray(r, dtype=np.float32)
    bf = np.ascontiguousarray(np.asarray(backfacing) != 0, dtype=np.uint8)
    if rr.shape != (n, spp) or bf.shape != (n, spp):
        raise ValueError("probe_depth_fold: r and backfacing have shape (%d, %d), not %s and %s" % (n, spp, rr.shape, bf.shape))
    if (moments is None) != (counts is None):
        raise ValueError("probe_depth_fold: moments and counts come together")
    acc = moments is not None
    m = np.array(moments, dtype=np.float32).reshape(-1, PROBE_DEPTH_ROW) if acc else np.zeros((n, PROBE_DEPTH_ROW), np.float32)
    c = np.array(counts, dtype=np.int32).reshape(-1, 2) if acc else np.zeros((n, 2), np.int32)
    if len(m) != n or len(c) != n:
        raise ValueError("probe_depth_fold: moments has shape (%d, %d) and counts (%d, 2)" % (n, PROBE_DEPTH_ROW, n))
    m, c = np.ascontiguousarray(m), np.ascontiguousarray(c)
    _check(lib().mcpt_probe_depth_fold_host(n, spp, _ptr(d), _ptr(rr), _ptr(bf), 1 if acc else 0, _ptr(m), _ptr(c)))
    return m, c


def probe_relight_fold(dirs, values, hysteresis=0.0, prev=None):
    """mcpt_probe_relight_fold_host (host only): the projection fold and the hysteresis blend of include/mcpt.h over given samples -- dirs
    (n, spp, 3), values (n, spp, 3), prev (n, 27) (required unless hysteresis is 0) -> (n, 27) float32.  The inputs are not changed."""
    d = np.ascontiguousarray(dirs, dtype=np.float32)
    if d.ndim != 3 or d.shape[2] != 3 or d.shape[1] < 1:
        raise ValueError("probe_relight_fold: dirs has shape (n, spp, 3) with spp >= 1, not %s" % (d.shape,))
    n, spp = d.shape[0], d.shape[1]
    v = np.ascontiguousarray(values, dtype=np.float32)
    if v.shape != d.shape:
        raise ValueError("probe_relight_fold: values has the shape of dirs %s, not %s" % (d.shape, v.shape))
    h = np.float32(hysteresis)
    if not (h >= 0 and h < 1):
        raise ValueError("probe_relight_fold: hysteresis is in [0, 1) as a float32, not %r" % (hysteresis,))
    p = None
    if prev is not None:
        p = np.ascontiguousarray(prev, dtype=np.float32)
        if p.shape != (n, 27):
            raise ValueError("probe_relight_fold: prev has shape (%d, 27), not %s" % (n, p.shape))
    elif h != 0:
        raise ValueError("probe_relight_fold: a hysteresis needs prev")
    out = np.zeros((n, 27), np.float32)
    _check(lib().mcpt_probe_relight_fold_host(n, spp, _ptr(d), _ptr(v), C.c_float(float(h)), _ptr(p) if p is not None else None, _ptr(out)))
    return out


def probe_shade_visible(origin, spacing, dims, sh, moments, counts, points, normals, normal_bias=0.0, backface_max=0.25, weight=False):
    """mcpt_probe_shade_visible_host (host only): the occlusion-aware grid lookup of include/mcpt.h -> (n, 3) float32, or (that, the
    summed weights A (n,)) with weight=True.  sh (probes, 27), moments (probes, 192), counts (probes, 2) int32."""
    who = "probe_shade_visible"
    g, m = _probe_grid(who, origin, spacing, dims)
    o = _probe_visibility(who, normal_bias, backface_max)
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    L = np.ascontiguousarray(sh, dtype=np.float32)
    M = np.ascontiguousarray(moments, dtype=np.float32)
    cn = np.ascontiguousarray(counts, dtype=np.int32)
    if L.shape != (m, 27) or M.shape != (m, PROBE_DEPTH_ROW) or cn.shape != (m, 2) or len(nr) != len(p) or m > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
        raise ValueError("%s: sh, moments and counts have shape (%d, 27), (%d, %d) and (%d, 2), with at most (2^31 - 1) / 192 probes, and there is "
                         "one normal per point, not %s, %s, %s, %d and %d" % (who, m, m, PROBE_DEPTH_ROW, m, L.shape, M.shape, cn.shape, len(nr), len(p)))
    out = np.zeros((len(p), 3), np.float32)
    wt = np.zeros(len(p), np.float32)
    _check(lib().mcpt_probe_shade_visible_host(C.byref(g), _ptr(L), _ptr(M), _ptr(cn), C.byref(o), len(p), _ptr(p), _ptr(nr), _ptr(out), _ptr(wt)))
    return (out, wt) if weight else out


def cull_bound(camera, root_min, root_max, library=None):
    """mcpt_cull_bound (host only): the sky cull's bound for a camera (scenes.CAM_DTYPE) over a root box, as a dict of mcpt_cull_info."""
    cam = np.ascontiguousarray(camera)
    lo, hi = np.ascontiguousarray(root_min, dtype=np.float32).reshape(3), np.ascontiguousarray(root_max, dtype=np.float32).reshape(3)
    info = CullInfo()
    L = lib(library)
    _check(L.mcpt_cull_bound(_ptr(cam), _ptr(lo), _ptr(hi), C.byref(info)), L=L)
    return info.as_dict()


def bvh_dump(sd):
    """Host-only (no GPU): the traversal tree mcpt_scene_create would build. Returns (info dict, boxes[n,12], children[n,2], qboxes[n,12] or None)."""
    keep = []
    d = _make_desc(sd, keep)
    info = BvhInfo()
    _check(lib().mcpt_bvh_dump(C.byref(d), C.byref(info), None, None, None, None, None))
    n = info.n_nodes
    boxes = np.zeros((n, 12), np.float32)
    children = np.zeros((n, 2), np.int32)
    qboxes = np.zeros((n, 12), np.uint16)
    shift, root_first = np.zeros((info.n_instances, 3), np.float32), np.zeros((info.n_instances, 2), np.int32)
    _check(lib().mcpt_bvh_dump(C.byref(d), C.byref(info), _ptr(boxes), _ptr(children), _ptr(qboxes), _ptr(shift), _ptr(root_first)))
    return _bvh_info_dict(info, shift, root_first), boxes, children, (qboxes if info.quantised else None)


def _bvh_info_dict(info, shift, root_first):
    out = {k: (list(getattr(info, k)) if k in ("root_min", "root_max", "q_origin", "q_cell") else getattr(info, k)) for k, _ in info._fields_}
    out["inst_shift"], out["inst_root_first"] = shift, root_first
    return out


class HipScene:
    """A scene resident in the HBM of one GPU (mcpt_scene_create)."""

    def __init__(self, sd, device=-1, library=None, builder=None, quantise=-1, instancing=None):
        """library: path of an alternative build of the same ABI (the checking build); None = the product library.
        builder: None (mcpt_scene_create: environment / default) or "sah" | "reference" | "lbvh" | "ploc" (mcpt_scene_create_ex)."""
        self.sd = sd
        self.device = int(device)  # (-1: the current device)
        self._keep = []
        self.L = lib(library)
        d = _make_desc(sd, self._keep)
        h = C.c_void_p()
        self.h = None
        if builder is None and quantise == -1 and instancing is None:
            _check(self.L.mcpt_scene_create(C.byref(d), int(device), C.byref(h)), L=self.L)
        else:
            # instancing: None automatic, False never, True whenever a mesh repeats (MCPT_INSTANCING_*)
            opt = BuildOptions(builder=BUILDERS[builder or "default"], quantise=int(quantise),
                               instancing=0 if instancing is None else (2 if instancing else 1))
            _check(self.L.mcpt_scene_create_ex(C.byref(d), int(device), C.byref(opt), C.byref(h)), L=self.L)
        self.h = h

    def dump_bvh(self):
        """The traversal tree as it sits in HBM: (info dict, boxes[n,12], children[n,2], qboxes[n,12] or None)."""
        info = BvhInfo()
        _check(self.L.mcpt_scene_dump_bvh(self.h, C.byref(info), None, None, None, None, None), L=self.L)
        n = info.n_nodes
        boxes, children, qboxes = np.zeros((n, 12), np.float32), np.zeros((n, 2), np.int32), np.zeros((n, 12), np.uint16)
        shift, root_first = np.zeros((info.n_instances, 3), np.float32), np.zeros((info.n_instances, 2), np.int32)
        _check(self.L.mcpt_scene_dump_bvh(self.h, C.byref(info), _ptr(boxes), _ptr(children), _ptr(qboxes), _ptr(shift), _ptr(root_first)), L=self.L)
        return _bvh_info_dict(info, shift, root_first), boxes, children, (qboxes if info.quantised else None)

    def update(self, moves):
        """mcpt_scene_update: moves = an iterable of (object index, 3x4 array), absolute transforms of the creation-time geometry.  Afterwards
        the scene behaves like one created from the moved description with the same build options.  Returns mcpt_update_info as a dict."""
        arr, n = _moves(moves)
        info = UpdateInfo()
        _check(self.L.mcpt_scene_update(self.h, n, C.cast(arr, C.c_void_p), C.byref(info)), L=self.L)
        return info.as_dict()

    def deform(self, items):
        """mcpt_scene_deform: items = an iterable of (object index, vertices), the new base positions of mesh objects.  vertices: a
        C-contiguous float32 numpy array of shape (n_tri, 3, 3) or (n_tri * 9,); or a buffer in the memory of the scene's device, read in
        place (anything with __cuda_array_interface__, or with data_ptr() and is_cuda such as a torch tensor, or DevicePositions(ptr,
        n_tri)), which must be complete before the call.  Returns mcpt_update_info as a dict."""
        arr, n, keep = _vertex_items(items, _mesh_tri_counts(self.sd))
        info = UpdateInfo()
        _check(self.L.mcpt_scene_deform(self.h, n, C.cast(arr, C.c_void_p), C.byref(info)), L=self.L)
        del keep
        return info.as_dict()

    def set_materials(self, edits=(), assign=()):
        """mcpt_scene_set_materials: edits = an iterable of (material index, material record as in scenes.MAT_DTYPE), assign = an iterable of
        (object index, material index).  Afterwards the scene behaves like one created from the edited description; in place (path 2)
        unless an object starts or stops emitting light.  Returns mcpt_update_info as a dict."""
        ea, ne, aa, na = _material_lists(edits, assign)
        info = UpdateInfo()
        _check(self.L.mcpt_scene_set_materials(self.h, ne, C.cast(ea, C.c_void_p), na, C.cast(aa, C.c_void_p), C.byref(info)), L=self.L)
        return info.as_dict()

    def set_visibility(self, items):
        """mcpt_scene_set_visibility: items = an iterable of (object index, visible).  Hidden objects leave the tree and the light tables
        and keep their records and ids; afterwards the scene behaves like one created from compact_scene(current description, mask).
        Returns mcpt_update_info as a dict."""
        arr, n = _visibility_items(items)
        info = UpdateInfo()
        _check(self.L.mcpt_scene_set_visibility(self.h, n, C.cast(arr, C.c_void_p), C.byref(info)), L=self.L)
        return info.as_dict()

    def visibility(self):
        """mcpt_scene_get_visibility: (mask as a uint8 array with one entry per object, number of primitives in the tree)."""
        mask, n = np.zeros(len(self.sd.objects), np.uint8), C.c_int32(0)
        _check(self.L.mcpt_scene_get_visibility(self.h, len(mask), _ptr(mask), C.byref(n)), L=self.L)
        return mask, int(n.value)

    def add_objects(self, objects, triangles, materials=None):
        """mcpt_scene_add_objects: appends objects (records of scenes.OBJ_DTYPE; first_tri relative to `triangles`, material an index into
        the material table after the append), their triangles and, optionally, materials.  Afterwards the scene behaves like one created
        from extend_scene(current description, ...), and self.sd is the extended SceneData.  Returns (index of the first added object,
        mcpt_update_info as a dict)."""
        a, arrays = _addition(self.sd, objects, triangles, materials)
        info, first = UpdateInfo(), C.c_int32(-1)
        _check(self.L.mcpt_scene_add_objects(self.h, C.byref(a), C.byref(first), C.byref(info)), L=self.L)
        self.sd = extend_scene(self.sd, *arrays)
        return int(first.value), info.as_dict()

    def set_environment(self, background, env=None):
        """mcpt_scene_set_environment: the background colour and the environment map (an (h, w, 3) float32 array, or None for the constant
        colour).  Returns mcpt_update_info as a dict."""
        bg, w, h, px, keep = _environment(background, env)
        info = UpdateInfo()
        _check(self.L.mcpt_scene_set_environment(self.h, C.cast(bg, C.c_void_p), w, h, px, C.byref(info)), L=self.L)
        del keep
        return info.as_dict()

    def close(self):
        if getattr(self, "h", None):
            self.L.mcpt_scene_destroy(self.h)
            self.h = None

    def tonemap(self, fb):
        """Renderer.cpp:95-103 on the GPU: (H, W, 3) float32 -> (H, W, 4) uint8."""
        fb = np.ascontiguousarray(fb, dtype=np.float32)
        out = np.zeros(fb.shape[:-1] + (4,), dtype=np.uint8)
        _check(self.L.mcpt_tonemap(self.h, _ptr(fb), fb.size // 3, _ptr(out)), L=self.L)
        return out

    def debug_counters(self):
        out = np.zeros(16, dtype=np.uint64)
        _check(self.L.mcpt_debug_counters(self.h, _ptr(out)), L=self.L)
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        i = SceneInfo()
        _check(self.L.mcpt_scene_get_info(self.h, C.byref(i)), L=self.L)
        return {k: getattr(i, k) for k, _ in i._fields_}

    def ray_counts(self):
        """mcpt_scene_ray_counts: (traced, shared) continuation rays of the last render or cast_rays call."""
        t, s = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.mcpt_scene_ray_counts(self.h, C.byref(t), C.byref(s)), L=self.L)
        return int(t.value), int(s.value)

    def primary_conductor_counts(self):
        """mcpt_scene_primary_conductor_counts: (samples, rays) of the primary kernel's short path in the last render call."""
        n, r = C.c_uint64(0), C.c_uint64(0)
        _check(self.L.mcpt_scene_primary_conductor_counts(self.h, C.byref(n), C.byref(r)), L=self.L)
        return int(n.value), int(r.value)

    def params(self, spp=None, seed=1, spp_total=0, sample_offset=0, accumulate=0, tile_size=32, rank=0, nranks=1,
               n_dir_sample=None, spp_per_pass=0, pool_paths=0, max_depth=0):
        sd = self.sd
        return Params(spp=int(spp if spp is not None else sd.spp), spp_total=int(spp_total), sample_offset=int(sample_offset),
                      rr_rate=float(sd.rr_rate), n_dir_sample=int(n_dir_sample if n_dir_sample is not None else sd.n_dir_sample),
                      enable_shadow=int(sd.enable_shadow), seed=int(seed), accumulate=int(accumulate), tile_size=int(tile_size),
                      rank=int(rank), nranks=int(nranks), spp_per_pass=int(spp_per_pass), pool_paths=int(pool_paths),
                      max_depth=int(max_depth))

    def render(self, camera=None, fb=None, **kw):
        """Renderer::Render up to the float framebuffer: returns (fb[H,W,3] float32, Stats)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        if fb is None:
            fb = np.zeros((H, W, 3), dtype=np.float32)
        p = self.params(**kw)
        st = Stats()
        _check(self.L.mcpt_render(self.h, _ptr(cam), C.byref(p), _ptr(fb), C.byref(st)), L=self.L)
        return fb, st

    def render_adaptive(self, min_spp, threshold, rel_floor=1e-3, dilate=1, camera=None, **kw):
        """mcpt_render_adaptive: pixels stop at the first level S0 * 2^r whose estimate (include/mcpt.h) is at most `threshold`; params
        spp (keyword `spp`, default the scene's) is the maximum.  Every pixel equals render(spp=its count) bit for bit.
        Returns (fb[H,W,3] float32, spp[H,W] int32, err[H,W] float32, info dict, Stats)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        fb = np.zeros((H, W, 3), dtype=np.float32)
        spp = np.zeros((H, W), dtype=np.int32)
        err = np.zeros((H, W), dtype=np.float32)
        p = self.params(**kw)
        o = Adaptive(min_spp=int(min_spp), dilate=int(dilate), threshold=float(threshold), rel_floor=float(rel_floor))
        info = AdaptiveInfo()
        st = Stats()
        _check(self.L.mcpt_render_adaptive(self.h, _ptr(cam), C.byref(p), C.byref(o), _ptr(fb), _ptr(spp), _ptr(err), C.byref(info), C.byref(st)),
               L=self.L)
        return fb, spp, err, info.as_dict(), st

    def _guide(self, guide, H, W):
        if guide is None:
            return None
        guide = np.ascontiguousarray(guide, dtype=np.float32)
        if guide.size != H * W:
            raise ValueError("the guide %s does not describe one %dx%d frame" % (guide.shape, W, H))
        return guide

    def render_adaptive_guided(self, min_spp, threshold, guide=None, rel_floor=1e-3, dilate=1, camera=None, variance=True, **kw):
        """mcpt_render_adaptive_guided: render_adaptive with pixel m's threshold scaled by sqrt(guide[m]) where guide[m] >= 1 (guide[H,W]
        float32, e.g. history_len(...); None: the plain rule) and the luminance variance of each pixel's mean at its own count.
        Returns (fb[H,W,3], spp[H,W] int32, err[H,W], variance[H,W] or None, info dict, Stats)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        fb = np.zeros((H, W, 3), dtype=np.float32)
        spp = np.zeros((H, W), dtype=np.int32)
        err = np.zeros((H, W), dtype=np.float32)
        var = np.zeros((H, W), dtype=np.float32) if variance else None
        guide = self._guide(guide, H, W)
        p = self.params(**kw)
        o = Adaptive(min_spp=int(min_spp), dilate=int(dilate), threshold=float(threshold), rel_floor=float(rel_floor))
        info = AdaptiveInfo()
        st = Stats()
        _check(self.L.mcpt_render_adaptive_guided(self.h, _ptr(cam), C.byref(p), C.byref(o), None if guide is None else _ptr(guide), _ptr(fb), _ptr(spp),
                                                  _ptr(err), None if var is None else _ptr(var), C.byref(info), C.byref(st)), L=self.L)
        return fb, spp, err, var, info.as_dict(), st

    def render_adaptive_weighted(self, min_spp, threshold, history_weight=None, max_history=0, rel_floor=1e-3, dilate=1, camera=None, variance=True,
                                 **kw):
        """mcpt_render_adaptive_weighted: render_adaptive_guided with the weight mode of the guide.  history_weight[H,W] float32 holds the
        samples behind each pixel's history (history_weight(...); None: the plain rule); with n samples so far a pixel's threshold is scaled
        by sqrt((min(H, (max_history - 1) n) + n) / n), the effective length the weighted blend will give it.  max_history: the blend's (0:
        32).  Returns (fb[H,W,3], spp[H,W] int32, err[H,W], variance[H,W] or None, info dict, Stats)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        fb = np.zeros((H, W, 3), dtype=np.float32)
        spp = np.zeros((H, W), dtype=np.int32)
        err = np.zeros((H, W), dtype=np.float32)
        var = np.zeros((H, W), dtype=np.float32) if variance else None
        guide = self._guide(history_weight, H, W)
        p = self.params(**kw)
        o = Adaptive(min_spp=int(min_spp), dilate=int(dilate), threshold=float(threshold), rel_floor=float(rel_floor))
        info = AdaptiveInfo()
        st = Stats()
        _check(self.L.mcpt_render_adaptive_weighted(self.h, _ptr(cam), C.byref(p), C.byref(o), None if guide is None else _ptr(guide), int(max_history),
                                                    _ptr(fb), _ptr(spp), _ptr(err), None if var is None else _ptr(var), C.byref(info), C.byref(st)),
               L=self.L)
        return fb, spp, err, var, info.as_dict(), st

    def render_adaptive_denoised(self, min_spp, threshold, guide=None, rel_floor=1e-3, dilate=1, camera=None, aov_spp=0, iterations=0, sigma_l=0.0,
                                 sigma_n=0.0, sigma_z=0.0, specular_depth=0, **kw):
        """mcpt_render_adaptive_denoised: render_adaptive_guided, the AOVs of render_aovs(aov_spp, seed, specular_depth) and the filter of the
        three with each pixel's own variance.  Returns dict(fb, denoised [H,W,3], spp[H,W] int32, err, variance [H,W], aov[H,W,8],
        adaptive_info, info, stats)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        fb, den = np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W, 3), dtype=np.float32)
        spp = np.zeros((H, W), dtype=np.int32)
        err, var = np.zeros((H, W), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
        aov = np.zeros((H, W, 8), dtype=np.float32)
        guide = self._guide(guide, H, W)
        p = self.params(**kw)
        r = Adaptive(min_spp=int(min_spp), dilate=int(dilate), threshold=float(threshold), rel_floor=float(rel_floor))
        o = denoise_opts(aov_spp, iterations, sigma_l, sigma_n, sigma_z, specular_depth)
        ainfo, info, st = AdaptiveInfo(), DenoiseInfo(), Stats()
        _check(self.L.mcpt_render_adaptive_denoised(self.h, _ptr(cam), C.byref(p), C.byref(r), None if guide is None else _ptr(guide), C.byref(o),
                                                    _ptr(fb), _ptr(den), _ptr(spp), _ptr(err), _ptr(var), _ptr(aov), C.byref(ainfo), C.byref(info),
                                                    C.byref(st)), L=self.L)
        return dict(fb=fb, denoised=den, spp=spp, err=err, variance=var, aov=aov, adaptive_info=ainfo.as_dict(), info=info.as_dict(), stats=st)

    def history_len(self, motion, prev_color, prev_depth, prev_len, normal=None, prev_normal=None, normal_test=False, normal_min=0.0, **opts):
        """mcpt_temporal_history_len: the out_len temporal_accumulate_ex will give every pixel whose new colour is finite, from what is known
        before the frame is rendered (motion[H,W,4], the previous history: prev_color[H,W,3], prev_depth, prev_len [H,W]; with normal_test
        the first-hit normals of both frames).  opts: max_history, depth_tol.  Returns len[H,W] float32."""
        motion = np.ascontiguousarray(motion, dtype=np.float32)
        H, W = motion.shape[:2]
        prev_color, prev_depth, prev_len = (np.ascontiguousarray(x, dtype=np.float32) for x in (prev_color, prev_depth, prev_len))
        normal, prev_normal = (None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (normal, prev_normal))
        n = H * W
        if (motion.size != n * 4 or prev_color.size != n * 3 or prev_depth.size != n or prev_len.size != n
                or any(x is not None and x.size != n * 3 for x in (normal, prev_normal))):
            raise ValueError("history_len: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W), dtype=np.float32)
        o = temporal_opts(**opts)
        ho = history_opts(normal_test, False, normal_min, 0.0)
        _check(self.L.mcpt_temporal_history_len(self.h, W, H, _ptr(motion), None if normal is None else _ptr(normal), _ptr(prev_color), _ptr(prev_depth),
                                                _ptr(prev_len), None if prev_normal is None else _ptr(prev_normal), C.byref(o), C.byref(ho), _ptr(out)),
               L=self.L)
        return out

    def history_weight(self, motion, prev_color, prev_depth, prev_len, prev_weight, normal=None, prev_normal=None, normal_test=False, normal_min=0.0,
                       **opts):
        """mcpt_temporal_history_weight: the history weight every pixel is about to get in temporal_accumulate_weighted (the smallest
        prev_weight of the taps it will use; 0 without history), from what is known before the frame is rendered: the arguments of
        history_len and prev_weight[H,W].  Returns weight[H,W] float32."""
        motion = np.ascontiguousarray(motion, dtype=np.float32)
        H, W = motion.shape[:2]
        prev_color, prev_depth, prev_len, prev_weight = (np.ascontiguousarray(x, dtype=np.float32) for x in (prev_color, prev_depth, prev_len, prev_weight))
        normal, prev_normal = (None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (normal, prev_normal))
        n = H * W
        if (motion.size != n * 4 or prev_color.size != n * 3 or prev_depth.size != n or prev_len.size != n or prev_weight.size != n
                or any(x is not None and x.size != n * 3 for x in (normal, prev_normal))):
            raise ValueError("history_weight: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W), dtype=np.float32)
        o = temporal_opts(**opts)
        ho = history_opts(normal_test, False, normal_min, 0.0)
        _check(self.L.mcpt_temporal_history_weight(self.h, W, H, _ptr(motion), None if normal is None else _ptr(normal), _ptr(prev_color),
                                                   _ptr(prev_depth), _ptr(prev_len), None if prev_normal is None else _ptr(prev_normal),
                                                   _ptr(prev_weight), C.byref(o), C.byref(ho), _ptr(out)), L=self.L)
        return out

    def render_aovs(self, aov_spp=0, seed=1, camera=None, specular_depth=0, centre=False, features=None):
        """mcpt_render_aovs: aov[H,W,8] float32 = {albedo rgb, normal xyz, depth, coverage} from feature samples 0 .. aov_spp-1 (0: 4) of `seed`;
        specular_depth > 0: mcpt_render_aovs_ex, the features taken behind up to that many mirror / glass bounces.
        centre: mcpt_render_aovs_features with centre 1, the features of each pixel's centre ray (aov_spp 0 or 1; `seed` is ignored).
        features: a FeatureOpts passed to mcpt_render_aovs_features as it is, or "null" for a null pointer (tests: either must give
        mcpt_render_aovs_ex's record)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        aov = np.zeros((H, W, 8), dtype=np.float32)
        if centre and features is None:
            features = FeatureOpts(centre=1)
        if features is not None:
            _check(self.L.mcpt_render_aovs_features(self.h, _ptr(cam), int(seed), int(aov_spp), int(specular_depth),
                                                    None if isinstance(features, str) else C.byref(features), _ptr(aov)), L=self.L)
        elif specular_depth == 0:
            _check(self.L.mcpt_render_aovs(self.h, _ptr(cam), int(seed), int(aov_spp), _ptr(aov)), L=self.L)
        else:
            _check(self.L.mcpt_render_aovs_ex(self.h, _ptr(cam), int(seed), int(aov_spp), int(specular_depth), _ptr(aov)), L=self.L)
        return aov

    def denoise(self, color, variance, aov, **opts):
        """mcpt_denoise: color[H,W,3], variance[H,W] (luminance variance of each colour mean), aov[H,W,8] -> out[H,W,3] float32.
        opts: iterations, sigma_l, sigma_n, sigma_z (0 = default; see include/mcpt.h)."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        aov = np.ascontiguousarray(aov, dtype=np.float32)
        if variance.size != H * W or aov.size != H * W * 8 or color.size != H * W * 3:
            raise ValueError("denoise: shapes %s %s %s do not describe one %dx%d frame" % (color.shape, variance.shape, aov.shape, W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        o = denoise_opts(**opts)
        _check(self.L.mcpt_denoise(self.h, W, H, _ptr(color), _ptr(variance), _ptr(aov), C.byref(o), _ptr(out)), L=self.L)
        return out

    def denoise_feedback(self, color, variance, aov, iteration=1, feedback=None, **opts):
        """mcpt_denoise_feedback: denoise(), and the history a feedback sequence keeps: the filter's records after a-trous iteration
        `iteration` (1..iterations), remodulated, with their variance.  Returns (out[H,W,3], fb_color[H,W,3], fb_variance[H,W]) float32.
        feedback: a FeedbackOpts passed as it is, or "null" for a null pointer (tests: a null or zeroed one must give mcpt_denoise and
        leave the feedback arrays, returned as zeros, untouched)."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        variance = np.ascontiguousarray(variance, dtype=np.float32)
        aov = np.ascontiguousarray(aov, dtype=np.float32)
        if variance.size != H * W or aov.size != H * W * 8 or color.size != H * W * 3:
            raise ValueError("denoise_feedback: shapes %s %s %s do not describe one %dx%d frame" % (color.shape, variance.shape, aov.shape, W, H))
        out, fc, fv = np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W, 3), dtype=np.float32), np.zeros((H, W), dtype=np.float32)
        o = denoise_opts(**opts)
        if feedback is None:
            feedback = FeedbackOpts(iteration=int(iteration))
        _check(self.L.mcpt_denoise_feedback(self.h, W, H, _ptr(color), _ptr(variance), _ptr(aov), C.byref(o),
                                            None if isinstance(feedback, str) else C.byref(feedback), _ptr(out), _ptr(fc), _ptr(fv)), L=self.L)
        return out, fc, fv

    def render_denoised(self, camera=None, aov_spp=0, iterations=0, sigma_l=0.0, sigma_n=0.0, sigma_z=0.0, features=True, specular_depth=0, **kw):
        """mcpt_render_denoised: the frame of render(**kw) (bit for bit), its luminance variance, the AOVs of render_aovs(aov_spp, seed, specular_depth) and
        the denoised frame.  Returns dict(fb[H,W,3], denoised[H,W,3], variance[H,W], aov[H,W,8], info dict, stats); features=False leaves
        the variance and the AOVs on the device (None here: 36 bytes per pixel less to copy)."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        fb = np.zeros((H, W, 3), dtype=np.float32)
        den = np.zeros((H, W, 3), dtype=np.float32)
        var = np.zeros((H, W), dtype=np.float32) if features else None
        aov = np.zeros((H, W, 8), dtype=np.float32) if features else None
        p = self.params(**kw)
        o = denoise_opts(aov_spp, iterations, sigma_l, sigma_n, sigma_z, specular_depth)
        info = DenoiseInfo()
        st = Stats()
        _check(self.L.mcpt_render_denoised(self.h, _ptr(cam), C.byref(p), C.byref(o), _ptr(fb), _ptr(den), None if var is None else _ptr(var),
                                           None if aov is None else _ptr(aov), C.byref(info),
                                           C.byref(st)), L=self.L)
        return dict(fb=fb, denoised=den, variance=var, aov=aov, info=info.as_dict(), stats=st)

    def snapshot(self):
        """mcpt_scene_snapshot: remembers where the geometry is now, as the "previous" positions of render_motion (valid across any number of
        update calls; without one, render_motion sees camera motion only)."""
        _check(self.L.mcpt_scene_snapshot(self.h), L=self.L)

    def render_motion(self, prev_camera=None, seed=1, aov_spp=0, camera=None, specular_depth=0, centre=False, features=None):
        """mcpt_render_motion: motion[H,W,4] float32 = {dx, dy, prev_depth, valid}: where the surface seen in each pixel was on the screen of
        prev_camera (default: the camera itself) when snapshot() was last called, from the feature samples of render_aovs(aov_spp, seed).
        specular_depth > 0: mcpt_render_motion_ex, the motion of what is seen behind up to that many mirror / glass bounces (the chains of
        render_aovs(aov_spp, seed, specular_depth=...)), as a virtual point on the primary ray.
        centre: mcpt_render_motion_features with centre 1, the motion of what each pixel's centre ray sees (aov_spp 0 or 1; `seed` is
        ignored); features: a FeatureOpts or "null", as in render_aovs."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        prev = np.ascontiguousarray(prev_camera if prev_camera is not None else cam)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        motion = np.zeros((H, W, 4), dtype=np.float32)
        if centre and features is None:
            features = FeatureOpts(centre=1)
        if features is not None:
            _check(self.L.mcpt_render_motion_features(self.h, _ptr(cam), _ptr(prev), int(seed), int(aov_spp), int(specular_depth),
                                                      None if isinstance(features, str) else C.byref(features), _ptr(motion)), L=self.L)
        elif specular_depth == 0:
            _check(self.L.mcpt_render_motion(self.h, _ptr(cam), _ptr(prev), int(seed), int(aov_spp), _ptr(motion)), L=self.L)
        else:
            _check(self.L.mcpt_render_motion_ex(self.h, _ptr(cam), _ptr(prev), int(seed), int(aov_spp), int(specular_depth), _ptr(motion)), L=self.L)
        return motion

    def temporal_blend(self, color, motion, prev_color, prev_depth, prev_len, **opts):
        """mcpt_temporal_blend: color[H,W,3] the new frame, motion[H,W,4] (render_motion), prev_color[H,W,3] / prev_len[H,W] the previous
        result of this call (prev_len 0 everywhere at the start), prev_depth[H,W] the depth channel of the previous frame's AOVs.
        opts: max_history, depth_tol (0 = default; see include/mcpt.h).  Returns (out[H,W,3], out_len[H,W]) float32."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        motion = np.ascontiguousarray(motion, dtype=np.float32)
        prev_color = np.ascontiguousarray(prev_color, dtype=np.float32)
        prev_depth = np.ascontiguousarray(prev_depth, dtype=np.float32)
        prev_len = np.ascontiguousarray(prev_len, dtype=np.float32)
        if color.size != H * W * 3 or motion.size != H * W * 4 or prev_color.size != H * W * 3 or prev_depth.size != H * W or prev_len.size != H * W:
            raise ValueError("temporal_blend: shapes %s %s %s %s %s do not describe one %dx%d frame"
                             % (color.shape, motion.shape, prev_color.shape, prev_depth.shape, prev_len.shape, W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        out_len = np.zeros((H, W), dtype=np.float32)
        o = temporal_opts(**opts)
        _check(self.L.mcpt_temporal_blend(self.h, W, H, _ptr(color), _ptr(motion), _ptr(prev_color), _ptr(prev_depth), _ptr(prev_len), C.byref(o),
                                          _ptr(out), _ptr(out_len)), L=self.L)
        return out, out_len

    def temporal_accumulate(self, color, variance, motion, prev_color, prev_variance, prev_depth, prev_len, **opts):
        """mcpt_temporal_accumulate: temporal_blend with the variance of its result.  variance[H,W] is the new frame's luminance variance of the
        colour mean (render_denoised), prev_variance[H,W] the previous out_variance of this call.  Returns (out[H,W,3], out_variance[H,W],
        out_len[H,W]) float32; out and out_len are temporal_blend's bit for bit."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        variance, motion, prev_color, prev_variance, prev_depth, prev_len = (
            np.ascontiguousarray(x, dtype=np.float32) for x in (variance, motion, prev_color, prev_variance, prev_depth, prev_len))
        n = H * W
        if (color.size != n * 3 or variance.size != n or motion.size != n * 4 or prev_color.size != n * 3 or prev_variance.size != n
                or prev_depth.size != n or prev_len.size != n):
            raise ValueError("temporal_accumulate: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        out_var = np.zeros((H, W), dtype=np.float32)
        out_len = np.zeros((H, W), dtype=np.float32)
        o = temporal_opts(**opts)
        _check(self.L.mcpt_temporal_accumulate(self.h, W, H, _ptr(color), _ptr(variance), _ptr(motion), _ptr(prev_color), _ptr(prev_variance),
                                               _ptr(prev_depth), _ptr(prev_len), C.byref(o), _ptr(out), _ptr(out_var), _ptr(out_len)), L=self.L)
        return out, out_var, out_len

    def temporal_accumulate_ex(self, color, variance, motion, normal, prev_color, prev_variance, prev_depth, prev_len, prev_normal,
                               normal_test=False, color_clamp=False, normal_min=0.0, clamp_k=0.0, **opts):
        """mcpt_temporal_accumulate_ex: temporal_accumulate with history rejection.  normal[H,W,3] / prev_normal[H,W,3] are the first-hit
        normals (render_aovs(...)[..., 3:6]) of this frame and of the previous one; both may be None unless normal_test is on.  Returns
        (out[H,W,3], out_variance[H,W], out_len[H,W] float32, flags[H,W] uint8: FLAG_NORMAL the normal test skipped a tap, FLAG_CLAMP the
        clamp moved the history).  With both switches off the first three are temporal_accumulate's bit for bit."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        variance, motion, prev_color, prev_variance, prev_depth, prev_len = (
            np.ascontiguousarray(x, dtype=np.float32) for x in (variance, motion, prev_color, prev_variance, prev_depth, prev_len))
        normal, prev_normal = (None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (normal, prev_normal))
        n = H * W
        if (color.size != n * 3 or variance.size != n or motion.size != n * 4 or prev_color.size != n * 3 or prev_variance.size != n
                or prev_depth.size != n or prev_len.size != n or any(x is not None and x.size != n * 3 for x in (normal, prev_normal))):
            raise ValueError("temporal_accumulate_ex: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        out_var = np.zeros((H, W), dtype=np.float32)
        out_len = np.zeros((H, W), dtype=np.float32)
        flags = np.zeros((H, W), dtype=np.uint8)
        o = temporal_opts(**opts)
        ho = history_opts(normal_test, color_clamp, normal_min, clamp_k)
        _check(self.L.mcpt_temporal_accumulate_ex(self.h, W, H, _ptr(color), _ptr(variance), _ptr(motion), None if normal is None else _ptr(normal),
                                                  _ptr(prev_color), _ptr(prev_variance), _ptr(prev_depth), _ptr(prev_len),
                                                  None if prev_normal is None else _ptr(prev_normal), C.byref(o), C.byref(ho), _ptr(out), _ptr(out_var),
                                                  _ptr(out_len), _ptr(flags)), L=self.L)
        return out, out_var, out_len, flags

    def temporal_accumulate_weighted(self, color, variance, motion, normal, count, prev_color, prev_variance, prev_depth, prev_len, prev_normal,
                                     prev_weight, normal_test=False, color_clamp=False, normal_min=0.0, clamp_k=0.0, **opts):
        """mcpt_temporal_accumulate_weighted: temporal_accumulate_ex with the history weighted by sample counts.  count: an int32 [H,W] array
        of this frame's per-pixel sample counts, or a number, the count of every pixel; prev_weight[H,W]: the previous out_weight of this
        call (0 for the first frame).  Returns (out[H,W,3], out_variance[H,W], out_len[H,W] float32, flags[H,W] uint8, out_weight[H,W]
        float32).  With one count for every pixel and frame the first four are temporal_accumulate_ex's bit for bit."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        variance, motion, prev_color, prev_variance, prev_depth, prev_len, prev_weight = (
            np.ascontiguousarray(x, dtype=np.float32) for x in (variance, motion, prev_color, prev_variance, prev_depth, prev_len, prev_weight))
        normal, prev_normal = (None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (normal, prev_normal))
        counts = None if np.isscalar(count) else np.ascontiguousarray(count, dtype=np.int32)
        n = H * W
        if (color.size != n * 3 or variance.size != n or motion.size != n * 4 or prev_color.size != n * 3 or prev_variance.size != n
                or prev_depth.size != n or prev_len.size != n or prev_weight.size != n or (counts is not None and counts.size != n)
                or any(x is not None and x.size != n * 3 for x in (normal, prev_normal))):
            raise ValueError("temporal_accumulate_weighted: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        out_var, out_len, out_weight = (np.zeros((H, W), dtype=np.float32) for _ in range(3))
        flags = np.zeros((H, W), dtype=np.uint8)
        o = temporal_opts(**opts)
        ho = history_opts(normal_test, color_clamp, normal_min, clamp_k)
        _check(self.L.mcpt_temporal_accumulate_weighted(self.h, W, H, _ptr(color), _ptr(variance), _ptr(motion), None if normal is None else _ptr(normal),
                                                        None if counts is None else _ptr(counts), 0.0 if counts is not None else float(count),
                                                        _ptr(prev_color), _ptr(prev_variance), _ptr(prev_depth), _ptr(prev_len),
                                                        None if prev_normal is None else _ptr(prev_normal), _ptr(prev_weight), C.byref(o), C.byref(ho),
                                                        _ptr(out), _ptr(out_var), _ptr(out_len), _ptr(flags), _ptr(out_weight)), L=self.L)
        return out, out_var, out_len, flags, out_weight

    def temporal_accumulate_moments(self, color, motion, normal, prev_color, prev_depth, prev_len, prev_normal, prev_moments, normal_test=False,
                                    color_clamp=False, normal_min=0.0, clamp_k=0.0, **opts):
        """mcpt_temporal_accumulate_moments: temporal_accumulate_ex without its variance planes, carrying the running first and second moment
        of each pixel's luminance instead.  prev_moments[H,W,2]: the previous out_moments of this call (0 for the first frame).  Returns
        (out[H,W,3], out_len[H,W] float32, flags[H,W] uint8, out_moments[H,W,2] float32); the first three are temporal_accumulate_ex's
        bit for bit."""
        color = np.ascontiguousarray(color, dtype=np.float32)
        H, W = color.shape[:2]
        motion, prev_color, prev_depth, prev_len, prev_moments = (
            np.ascontiguousarray(x, dtype=np.float32) for x in (motion, prev_color, prev_depth, prev_len, prev_moments))
        normal, prev_normal = (None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in (normal, prev_normal))
        n = H * W
        if (color.size != n * 3 or motion.size != n * 4 or prev_color.size != n * 3 or prev_depth.size != n or prev_len.size != n
                or prev_moments.size != n * 2 or any(x is not None and x.size != n * 3 for x in (normal, prev_normal))):
            raise ValueError("temporal_accumulate_moments: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W, 3), dtype=np.float32)
        out_len = np.zeros((H, W), dtype=np.float32)
        flags = np.zeros((H, W), dtype=np.uint8)
        out_moments = np.zeros((H, W, 2), dtype=np.float32)
        o = temporal_opts(**opts)
        ho = history_opts(normal_test, color_clamp, normal_min, clamp_k)
        _check(self.L.mcpt_temporal_accumulate_moments(self.h, W, H, _ptr(color), _ptr(motion), None if normal is None else _ptr(normal),
                                                       _ptr(prev_color), _ptr(prev_depth), _ptr(prev_len),
                                                       None if prev_normal is None else _ptr(prev_normal), _ptr(prev_moments), C.byref(o),
                                                       C.byref(ho), _ptr(out), _ptr(out_len), _ptr(flags), _ptr(out_moments)), L=self.L)
        return out, out_len, flags, out_moments

    def moments_variance(self, moments, len, aov, flags=None, min_len=0, radius=0, sigma_z=0.0):
        """mcpt_moments_variance: variance[H,W] float32 of the accumulated frame's luminance from its moments[H,W,2] and history lengths
        len[H,W] (temporal_accumulate_moments' outputs), that frame's flags[H,W] uint8 (None: no pixel counts as clamped) and the AOVs
        aov[H,W,8] the filter will read: temporal where the history has min_len frames, a gated spatial estimate elsewhere."""
        moments = np.ascontiguousarray(moments, dtype=np.float32)
        H, W = moments.shape[:2]
        len, aov = (np.ascontiguousarray(x, dtype=np.float32) for x in (len, aov))
        flags = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8)
        n = H * W
        if moments.size != n * 2 or len.size != n or aov.size != n * 8 or (flags is not None and flags.size != n):
            raise ValueError("moments_variance: the arrays do not describe one %dx%d frame" % (W, H))
        out = np.zeros((H, W), dtype=np.float32)
        o = moments_opts(True, min_len, radius, sigma_z)
        _check(self.L.mcpt_moments_variance(self.h, W, H, _ptr(moments), _ptr(len), None if flags is None else _ptr(flags), _ptr(aov), C.byref(o),
                                            _ptr(out)), L=self.L)
        return out

    def sequence(self, width=None, height=None, filter=True, max_history=0, depth_tol=0.0, normal_test=False, color_clamp=False, normal_min=0.0,
                 clamp_k=0.0, adaptive=None, specular_motion=False, weighted=False, moments=False, centre_features=False, feedback=0,
                 **denoise_opts_kw):
        """mcpt_sequence_create: a HipSequence of width x height frames (default: the scene camera's) on this scene.  filter: also denoise
        the accumulated frame; max_history, depth_tol: mcpt_temporal_opts; the rest: mcpt_denoise_opts (aov_spp, iterations, sigma_l,
        sigma_n, sigma_z, specular_depth).  normal_test / color_clamp (normal_min, clamp_k): history rejection, mcpt_history_opts; with
        either on the sequence is made by mcpt_sequence_create_ex and HipSequence.flags() tells what the last frame rejected.
        adaptive: dict(min_spp=, threshold=, rel_floor=, dilate=, guided=) (the keywords of sequence_adaptive): the frames are adaptive
        (mcpt_sequence_create_adaptive), each frame's `spp` is the cap, and HipSequence.counts() gives the last frame's counts.
        specular_motion: with specular_depth > 0 the motion follows the mirror / glass chains too and the history is validated against the
        chain depth (mcpt_sequence_create_motion).
        weighted: the history is weighted by sample counts -- the count map of an adaptive frame, `spp` of a uniform one -- and a guided
        adaptive rule is guided by the history weight (mcpt_sequence_create_weighted); HipSequence.weight() gives the last frame's weights.
        moments: True or dict(min_len=, radius=, sigma_z=): the variance comes from the temporal moments of each pixel's luminance, carried
        in the history, and frames may have `spp` 1 (mcpt_sequence_create_moments); HipSequence.moments() gives the last frame's moments.
        centre_features: every feature pass of a frame (AOVs, motion) runs on the pixels' centre rays, one per pixel, so that a static
        pixel's features are the same bits in every frame whatever the seed and the lens (mcpt_sequence_create_features; aov_spp 0 or 1).
        feedback: k > 0 feeds the filter's a-trous iteration k back into the history the next frame blends with, as SVGF does
        (mcpt_sequence_create_feedback; needs filter, no adaptive rule, no weighting); HipSequence.history() gives that history.
        The sequence owns the scene's snapshot while it lives; close it before the scene."""
        return HipSequence(self, width, height, filter, max_history, depth_tol, normal_test=normal_test, color_clamp=color_clamp,
                           normal_min=normal_min, clamp_k=clamp_k, adaptive=adaptive, specular_motion=specular_motion, weighted=weighted,
                           moments=moments, features=FeatureOpts(centre=1) if centre_features else None,
                           feedback=FeedbackOpts(iteration=int(feedback)) if feedback else None, **denoise_opts_kw)

    def render_device(self, fb_ptr, stream_ptr=0, camera=None, **kw):
        """Same, into a device framebuffer (W*H*3 floats at fb_ptr) on the given hipStream_t handle."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        p = self.params(**kw)
        st = Stats()
        _check(self.L.mcpt_render_device(self.h, _ptr(cam), C.byref(p), C.c_void_p(int(fb_ptr)), C.c_void_p(int(stream_ptr)),
                                         C.byref(st)), L=self.L)
        return st

    MATERIAL_KINDS = {"eval": 0, "pdf": 1, "fresnel": 2, "sample": 3, "refract": 4, "eval_pdf": 5, "reflect": 6}

    def debug_material(self, kind, rows, sel):
        """The device's Material functions on arrays (mcpt_debug_material): rows [n, 13] = {a, b, c, uv, u1, u2}, sel [n, 3] =
        {material index, channel, is_reflect}; returns [n, 4]."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 13)
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1, 3)
        out = np.zeros((len(rows), 4), np.float32)
        _check(self.L.mcpt_debug_material(self.h, self.MATERIAL_KINDS[kind], len(rows), _ptr(rows), _ptr(sel), _ptr(out)), L=self.L)
        return out

    def sample_light(self, u):
        """The device's Scene::sampleLight for rows of four uniforms (mcpt_debug_scene) -> [n, 10] = {point, normal, emission, pdf}."""
        u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 4)
        out = np.zeros((len(u), 10), np.float32)
        _check(self.L.mcpt_debug_scene(self.h, 0, len(u), _ptr(u), _ptr(out)), L=self.L)
        return out

    def sample_env(self, dirs):
        """The device's Scene::sampleEnv for rows of directions -> [n, 3]."""
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(d), 3), np.float32)
        _check(self.L.mcpt_debug_scene(self.h, 1, len(d), _ptr(d), _ptr(out)), L=self.L)
        return out

    def intersect(self, origins, dirs):
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        n = len(o)
        t = np.zeros(n, dtype=np.float64)
        prim = np.zeros(n, dtype=np.int32)
        _check(self.L.mcpt_intersect(self.h, n, _ptr(o), _ptr(d), _ptr(t), _ptr(prim)), L=self.L)
        return t, prim

    def query_closest(self, origins, dirs, tmax=None, want=("t", "prim"), out=None, stream=None):
        """mcpt_query_closest: closest hits of rays that sit in the memory of the scene's device, enqueued on `stream` without a host
        synchronisation.  origins, dirs: float32, C-contiguous, shape (n, 3); tmax: (n,) or None (no limit; with one, a ray keeps its hit
        iff t - tmax <= -1e-4f).  Each is anything with __cuda_array_interface__, or with data_ptr() and is_cuda (a torch tensor).
        want: names among t, prim, object, uv, normal, point.  out: dict name -> device buffer (float64 (n,), int32 (n,), int32 (n,),
        float32 (n, 2), (n, 3), (n, 3)); it may be None when the inputs are torch tensors: the outputs are then torch.empty tensors on their
        device and the stream defaults to torch's current one.  Returns (dict name -> buffer, mcpt_query_info as a dict); the results are
        ready in stream order."""
        who = "query_closest"
        want = tuple(want)
        if not want or any(w not in QUERY_OUTPUTS for w in want) or len(set(want)) != len(want):
            raise ValueError("%s: want is a non-empty selection of %s without repeats, not %r" % (who, tuple(QUERY_OUTPUTS), want))
        n, rays = _query_rays(who, origins, dirs, tmax)
        spec = {w: (_row_shape(n, QUERY_OUTPUTS[w][1]), QUERY_OUTPUTS[w][0]) for w in want}
        out, ptrs, stream = _outputs(who, spec, out, _device_of(origins, dirs), stream)
        hits = HitBuffers(**{w: ptrs[w] or None for w in want})
        info = QueryInfo()
        _check(self.L.mcpt_query_closest(self.h, n, C.byref(rays), C.byref(hits), C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return {w: out[w] for w in want}, info.as_dict()

    def query_occluded(self, origins, dirs, tmax, out=None, stream=None):
        """mcpt_query_occluded: the any-hit query for rays in device memory -> (uint8 (n,) device buffer, mcpt_query_info as a dict):
        1 where some primitive is hit with t - tmax <= -1e-4f.  tmax = inf asks whether anything is hit.  Inputs, out and stream as in
        query_closest."""
        who = "query_occluded"
        if tmax is None:
            raise ValueError("%s: tmax is required" % who)
        n, rays = _query_rays(who, origins, dirs, tmax)
        out, ptrs, stream = _outputs(who, {None: ((n,), "uint8")}, out, _device_of(origins, dirs), stream)
        info = QueryInfo()
        _check(self.L.mcpt_query_occluded(self.h, n, C.byref(rays), C.c_void_p(ptrs[None]), C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return out, info.as_dict()

    def query_radiance(self, origins, dirs, kind="ray", variance=False, out=None, stream=None, **params):
        """mcpt_query_radiance: path-traced radiance at sensors that sit in the memory of the scene's device -> (radiance (n, 3), variance
        (n, 3) or None, Stats).  kind "ray": origins and dirs are rays, used as given; "hemisphere": surface points and unit normals, the
        result is the cosine-weighted mean of the incoming radiance (E / pi).  Sensor i is keyed like pixel i of a frame: the result is
        the fold of cast_rays(.., pixel=i, sample=sample_offset + k, channel=c) over the spp samples, bit for bit.  variance=True (spp >= 2,
        no progressive parameters): also the variance of each channel's mean.  Inputs, out and stream as in query_closest: out is a dict
        with "radiance" (and "variance") float32 (n, 3) device buffers, or None when the inputs are torch tensors.  params: the keywords
        of HipScene.params (spp, seed, sample_offset, spp_total, accumulate, spp_per_pass, pool_paths, ...).  The call blocks until the
        outputs are written."""
        who = "query_radiance"
        k = _sensor_kind(who, kind)
        n, rays = _query_rays(who, origins, dirs, None)
        names = ("radiance", "variance") if variance else ("radiance",)
        out, ptrs, stream = _outputs(who, {w: ((n, 3), "float32") for w in names}, out, _device_of(origins, dirs), stream)
        sensors = SensorBuffers(rays.origins, rays.dirs, k, (C.c_int32 * 3)(0, 0, 0))
        outs = SensorOutputs(ptrs["radiance"] or None, ptrs.get("variance") or None)
        p = self.params(**params)
        st = Stats()
        _check(self.L.mcpt_query_radiance(self.h, C.byref(p), n, C.byref(sensors), C.byref(outs), C.c_void_p(int(stream or 0)), C.byref(st)), L=self.L)
        return out["radiance"], (out["variance"] if variance else None), st

    def _torch_device(self):
        """The torch device of the scene (outputs the lightmap calls allocate themselves)."""
        import torch
        return torch.device("cuda", self.device if self.device >= 0 else torch.cuda.current_device())

    def lightmap_texels(self, object, width, height, flip_normals=False, want=("texel", "prim", "bary", "origins", "normals"), out=None, stream=None):
        """mcpt_lightmap_texels: the texel sensors of mesh `object` for a width x height map, from the scene as it is now -> (dict name ->
        buffer, n).  Row i < n describes covered texel texel[i] (ascending y*width + x): prim its owner, bary (u, v), origins the point on the
        live triangle, normals the live normal (negated with flip_normals): origins and normals are sensors for query_radiance(kind=
        "hemisphere").  want: names among texel, prim, bary, origins, normals ("texel" is always written).  out: dict name -> device buffer
        of width*height rows (int32 (N,), int32 (N,), float32 (N, 2), (N, 3), (N, 3)); None: torch tensors on the scene's device, returned
        cut to their first n rows, and the stream defaults to torch's current one.  Blocks until n is known."""
        who = "lightmap_texels"
        want = tuple(want)
        if any(w not in LIGHTMAP_OUTPUTS for w in want) or len(set(want)) != len(want):
            raise ValueError("%s: want is a selection of %s without repeats, not %r" % (who, tuple(LIGHTMAP_OUTPUTS), want))
        if "texel" not in want:
            want = ("texel",) + want
        d = _lightmap_desc(object, width, height, flip_normals)
        cap = max(int(width), 0) * max(int(height), 0)
        made = out is None
        rows = 0 if made and cap > (2 ** 31 - 1) // 3 else cap  # (the library refuses the size before it writes anything)
        spec = {w: (_row_shape(rows, LIGHTMAP_OUTPUTS[w][1]), LIGHTMAP_OUTPUTS[w][0]) for w in want}
        out, ptrs, stream = _outputs(who, spec, out, self._torch_device() if made else None, stream)
        bufs = LightmapTexelsOut(**{w: ptrs[w] or None for w in want})
        n = C.c_int64(0)
        _check(self.L.mcpt_lightmap_texels(self.h, C.byref(d), C.byref(bufs), C.byref(n), C.c_void_p(int(stream or 0))), L=self.L)
        return {w: (out[w][:n.value] if made else out[w]) for w in want}, int(n.value)

    def _lightmap_planes(self, who, width, height, out, names, stream):
        """The device addresses of the planes `names` (image / variance: float32 (height, width, 3); coverage: uint8 (height, width)) in
        `out`, torch tensors on the scene's device when out is None -> (out, {name: address}, stream)."""
        W, H = int(width), int(height)
        made = out is None
        if made and not (W >= 1 and H >= 1 and W * H <= (2 ** 31 - 1) // 3):
            H = W = 1  # (the library refuses the size before it writes anything)
        spec = {w: ((H, W), "uint8") if w == "coverage" else ((H, W, 3), "float32") for w in names}
        return _outputs(who, spec, out, self._torch_device() if made else None, stream)

    def lightmap_scatter(self, object, width, height, texel, values, dilate=2, coverage=True, out=None, stream=None):
        """mcpt_lightmap_scatter: image[texel[i]] = values[i] on a zero map, then `dilate` rounds of the dilation of include/mcpt.h ->
        (image (height, width, 3), coverage (height, width) uint8 or None).  texel: int32 (n,), values: float32 (n, 3); device buffers
        (torch tensors, __cuda_array_interface__) are read in place, numpy arrays are staged through torch.  out: dict with "image" (and
        "coverage") device buffers; None: torch tensors.  Enqueued on `stream` (default with torch inputs or outputs: torch's current one)."""
        who = "lightmap_scatter"
        bt, bv = _device_buffer(texel, who, "texel", "int32"), _device_buffer(values, who, "values")
        keep = []
        if bt is None or bv is None:
            import torch
            dev = self._torch_device()
            texel = torch.from_numpy(np.ascontiguousarray(texel, dtype=np.int32).reshape(-1)).to(dev)
            values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).reshape(-1, 3)).to(dev)
            keep = [texel, values]
            bt, bv = _device_buffer(texel, who, "texel", "int32"), _device_buffer(values, who, "values")
            if stream is None:
                stream = torch.cuda.current_stream(dev).cuda_stream
        if len(bt[1]) != 1 or bv[1] != (bt[1][0], 3):
            raise ValueError("%s: texel has shape (n,) and values (n, 3), not %s and %s" % (who, bt[1], bv[1]))
        if out is None and stream is None and _is_torch(texel, values):
            import torch
            stream = torch.cuda.current_stream(texel.device).cuda_stream
        names = ("image", "coverage") if coverage else ("image",)
        out, ptrs, stream = self._lightmap_planes(who, width, height, out, names, stream)
        d = _lightmap_desc(object, width, height)
        _check(self.L.mcpt_lightmap_scatter(self.h, C.byref(d), bt[1][0], C.c_void_p(bt[0] or 0), C.c_void_p(bv[0] or 0), int(dilate),
                                            C.c_void_p(ptrs["image"]), C.c_void_p(ptrs.get("coverage") or 0), C.c_void_p(int(stream or 0))), L=self.L)
        if keep:  # the staged inputs must outlive the kernels that read them
            import torch
            torch.cuda.synchronize(keep[0].device)
        return out["image"], (out["coverage"] if coverage else None)

    def bake_lightmap(self, object, width, height, dilate=2, variance=False, out=None, stream=None, flip_normals=False, **params):
        """mcpt_bake_lightmap: the lightmap of mesh `object` -- lightmap_texels, query_radiance(kind="hemisphere") at those sensors and
        lightmap_scatter in one call -> (image (height, width, 3), coverage (height, width) uint8, variance (height, width, 3) or None,
        mcpt_lightmap_info as a dict, Stats).  The image holds E / pi at covered texels, `dilate` rounds of dilation around them, 0
        elsewhere; the variance (spp >= 2) is that of each covered texel's mean, not dilated.  out: dict with "image", "coverage" (and
        "variance") device buffers; None: torch tensors on the scene's device.  params: the keywords of HipScene.params; sample_offset,
        spp_total and accumulate must stay 0.  The call blocks until the map is written."""
        who = "bake_lightmap"
        names = ("image", "coverage", "variance") if variance else ("image", "coverage")
        out, ptrs, stream = self._lightmap_planes(who, width, height, out, names, stream)
        d = _lightmap_desc(object, width, height, flip_normals)
        p = self.params(**params)
        info, st = LightmapInfo(), Stats()
        _check(self.L.mcpt_bake_lightmap(self.h, C.byref(d), C.byref(p), int(dilate), C.c_void_p(ptrs["image"]), C.c_void_p(ptrs["coverage"]),
                                         C.c_void_p(ptrs.get("variance") or 0), C.c_void_p(int(stream or 0)), C.byref(info), C.byref(st)), L=self.L)
        return out["image"], out["coverage"], (out["variance"] if variance else None), info.as_dict(), st

    def sensor_rays(self, kind, origins, dirs, sensor, sample, seed=1):
        """mcpt_sensor_rays: the first ray of (sensor[j], sample[j]) for sensors given on the host -> (origins[n,3], dirs[n,3]) float32.
        origins, dirs: a row per sensor; sample is absolute (sample_offset + k)."""
        k = _sensor_kind("sensor_rays", kind)
        po = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        pd = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        si = np.ascontiguousarray(sensor, dtype=np.uint32).reshape(-1)
        sm = np.ascontiguousarray(sample, dtype=np.uint32).reshape(-1)
        n = len(si)
        if len(sm) != n or len(po) != len(pd) or (n and int(si.max()) >= len(po)):
            raise ValueError("sensor_rays: sensor and sample have one length, and every sensor named has a row in origins and dirs")
        o = np.zeros((n, 3), dtype=np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        _check(self.L.mcpt_sensor_rays(self.h, k, int(seed), n, _ptr(po), _ptr(pd), _ptr(si), _ptr(sm), _ptr(o), _ptr(d)), L=self.L)
        return o, d

    def query_probes(self, origins, radiance=False, variance=False, out=None, stream=None, indirect_only=False, **params):
        """mcpt_query_probes: light probes at points (n, 3) in the memory of the scene's device -> (sh (n, 27), radiance (n, 3) or None,
        variance (n, 3) or None, Stats).  sh[i, 3j + c] is coefficient j of channel c of the incoming radiance over the whole sphere at
        point i, the fold of include/mcpt.h over the first rays probe_rays gives; radiance is the mean over the sphere.  Inputs, out and
        stream as in query_radiance: out is a dict with "sh" (and "radiance", "variance") float32 device buffers, or None when origins
        is a torch tensor.  params: the keywords of HipScene.params.  The call blocks until the outputs are written.  indirect_only
        (mcpt_query_probes_ex): a sample whose first ray hits an emitter contributes 0, the volume that goes with query_direct."""
        who = "query_probes"
        po, n = _rows(who, "origins", origins, 3)
        if n > (2 ** 31 - 1) // 27:
            raise ValueError("%s: at most (2^31 - 1) / 27 probes, not %d" % (who, n))
        names = ("sh",) + (("radiance",) if radiance or variance else ()) + (("variance",) if variance else ())
        spec = {w: ((n, 27 if w == "sh" else 3), "float32") for w in names}
        out, ptrs, stream = _outputs(who, spec, out, _device_of(origins), stream)
        outs = ProbeOutputs(ptrs["sh"] or None, ptrs.get("radiance") or None, ptrs.get("variance") or None, None)
        p = self.params(**params)
        st = Stats()
        _check(self.L.mcpt_query_probes_ex(self.h, C.byref(p), n, C.c_void_p(po or 0), C.byref(outs), C.c_void_p(int(stream or 0)), C.byref(st),
                                           _probe_opts(indirect_only)), L=self.L)
        return out["sh"], out.get("radiance") if "radiance" in names else None, (out["variance"] if variance else None), st

    def probe_rays(self, origins, sensor, sample, seed=1):
        """mcpt_probe_rays: the first ray of (probe sensor[j], sample[j]) for probes given on the host -> (origins[n,3], dirs[n,3]) float32;
        sample is absolute (sample_offset + k)."""
        po = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        si = np.ascontiguousarray(sensor, dtype=np.uint32).reshape(-1)
        sm = np.ascontiguousarray(sample, dtype=np.uint32).reshape(-1)
        n = len(si)
        if len(sm) != n or (n and int(si.max()) >= len(po)):
            raise ValueError("probe_rays: sensor and sample have one length, and every probe named has a row in origins")
        o = np.zeros((n, 3), dtype=np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        _check(self.L.mcpt_probe_rays(self.h, int(seed), n, _ptr(po), _ptr(si), _ptr(sm), _ptr(o), _ptr(d)), L=self.L)
        return o, d

    def probe_shade(self, origin, spacing, dims, sh, points, normals, out=None, stream=None):
        """mcpt_probe_shade: the grid lookup of include/mcpt.h on the device, E / pi at points (n, 3) for normals (n, 3) from the grid's
        coefficients sh (probes, 27) -> (n, 3) float32 device buffer.  All are device buffers; out may be None with torch inputs.  Enqueued
        on `stream` without a synchronisation."""
        who = "probe_shade"
        g, m = _probe_grid(who, origin, spacing, dims)
        ps = _device_array(who, "sh", sh, (m, 27))
        pp, n = _rows(who, "points", points, 3)
        pn = _device_array(who, "normals", normals, (n, 3))
        out, ptrs, stream = _outputs(who, {None: ((n, 3), "float32")}, out, _device_of(points, normals, sh), stream)
        _check(self.L.mcpt_probe_shade(self.h, C.byref(g), C.c_void_p(ps or 0), n, C.c_void_p(pp or 0), C.c_void_p(pn or 0), C.c_void_p(ptrs[None]),
                                       C.c_void_p(int(stream or 0))), L=self.L)
        return out

    def bake_probe_grid(self, origin, spacing, dims, out=None, stream=None, indirect_only=False, **params):
        """mcpt_bake_probe_grid: probe_grid_points on the device into a scene-owned buffer, then query_probes there -> (sh (probes, 27),
        Stats).  out: a float32 (probes, 27) device buffer; None: a torch tensor on the scene's device.  indirect_only: as for query_probes
        (mcpt_bake_probe_grid_ex)."""
        who = "bake_probe_grid"
        g, m = _probe_grid(who, origin, spacing, dims)
        out, ptrs, stream = _outputs(who, {None: ((m, 27), "float32")}, out, self._torch_device() if out is None else None, stream)
        p = self.params(**params)
        st = Stats()
        _check(self.L.mcpt_bake_probe_grid_ex(self.h, C.byref(g), C.byref(p), C.c_void_p(ptrs[None]), C.c_void_p(int(stream or 0)), C.byref(st),
                                              _probe_opts(indirect_only)), L=self.L)
        return out, st

    def query_probe_depth(self, origins, spp, max_distance, seed=1, sample_offset=0, accumulate=0, out=None, stream=None):
        """mcpt_query_probe_depth: the depth maps of probes at points (n, 3) in the memory of the scene's device -> (moments (n, 192)
        float32, counts (n, 2) int32, mcpt_query_info as a dict): per probe and texel of the 8 x 8 octahedral map the sums (W, S1, S2) of
        include/mcpt.h over the first rays probe_rays gives, and per probe its samples and how many of them hit a back face.  out: a dict
        with "moments" and "counts" device buffers (required with accumulate), or None when origins is a torch tensor.  Enqueued on
        `stream` without a synchronisation, through the staging buffers of the ray queries."""
        who = "query_probe_depth"
        po, n = _rows(who, "origins", origins, 3)
        if n > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
            raise ValueError("%s: at most (2^31 - 1) / 192 probes, not %d" % (who, n))
        p = _probe_depth_params(who, spp, max_distance, seed, sample_offset, accumulate)
        if out is None and p.accumulate:
            raise ValueError("%s: accumulate continues the buffers given in out" % who)
        spec = {"moments": ((n, PROBE_DEPTH_ROW), "float32"), "counts": ((n, 2), "int32")}
        out, ptrs, stream = _outputs(who, spec, out, _device_of(origins), stream)
        info = QueryInfo()
        _check(self.L.mcpt_query_probe_depth(self.h, C.byref(p), n, C.c_void_p(po or 0), C.c_void_p(ptrs["moments"]), C.c_void_p(ptrs["counts"]),
                                             C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return out["moments"], out["counts"], info.as_dict()

    def query_direct(self, points, normals, n_samples, seed=1, key_sample=0, out=None, stream=None):
        """mcpt_query_direct: the sampled direct term D of include/mcpt.h (E_direct / pi of a Lambertian surface) at points (n, 3) with unit
        normals (n, 3) in the memory of the scene's device, from n_samples light samples and shadow rays per point -> ((n, 3) float32
        device buffer, mcpt_query_info as a dict).  Point i draws with the Philox key (seed, i) and the sample word key_sample.  out may
        be None with torch inputs.  Enqueued on `stream` without a synchronisation, through the staging buffers of the ray queries."""
        who = "query_direct"
        pp, n = _rows(who, "points", points, 3)
        pn = _device_array(who, "normals", normals, (n, 3))
        if not 1 <= int(n_samples) <= DIRECT_MAX_SAMPLES:
            raise ValueError("%s: n_samples must be in 1 .. %d, not %r" % (who, DIRECT_MAX_SAMPLES, n_samples))
        if n * int(n_samples) > 2 ** 31 - 1:
            raise ValueError("%s: n * n_samples must be at most 2^31 - 1" % who)
        out, ptrs, stream = _outputs(who, {None: ((n, 3), "float32")}, out, _device_of(points, normals), stream)
        o = DirectOpts(seed=int(seed) & 0xffffffff, n_samples=int(n_samples), key_sample=int(key_sample) & 0xffffffff)
        info = QueryInfo()
        _check(self.L.mcpt_query_direct(self.h, C.byref(o), n, C.c_void_p(pp or 0), C.c_void_p(pn or 0), C.c_void_p(ptrs[None]),
                                        C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return out, info.as_dict()

    def probe_shade_visible(self, origin, spacing, dims, sh, moments, counts, points, normals, normal_bias=0.0, backface_max=0.25, weight=None,
                            out=None, stream=None):
        """mcpt_probe_shade_visible: the occlusion-aware grid lookup of include/mcpt.h on the device, E / pi at points (n, 3) for normals
        (n, 3) from the grid's coefficients sh (probes, 27), depth moments (probes, 192) and counts (probes, 2) -> (n, 3) float32 device
        buffer.  weight: an optional float32 (n,) device buffer for the summed weights A.  All are device buffers; out may be None with
        torch inputs.  Enqueued on `stream` without a synchronisation."""
        who = "probe_shade_visible"
        g, m = _probe_grid(who, origin, spacing, dims)
        if m > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
            raise ValueError("%s: at most (2^31 - 1) / 192 probes, not %d" % (who, m))
        o = _probe_visibility(who, normal_bias, backface_max)
        ps = _device_array(who, "sh", sh, (m, 27))
        pm = _device_array(who, "moments", moments, (m, PROBE_DEPTH_ROW))
        pc = _device_array(who, "counts", counts, (m, 2), "int32")
        pp, n = _rows(who, "points", points, 3)
        pn = _device_array(who, "normals", normals, (n, 3))
        pw = _device_array(who, "weight", weight, (n,)) if weight is not None else 0
        out, ptrs, stream = _outputs(who, {None: ((n, 3), "float32")}, out, _device_of(points, normals, sh, moments, counts), stream)
        _check(self.L.mcpt_probe_shade_visible(self.h, C.byref(g), C.c_void_p(ps or 0), C.c_void_p(pm or 0), C.c_void_p(pc or 0), C.byref(o), n,
                                               C.c_void_p(pp or 0), C.c_void_p(pn or 0), C.c_void_p(ptrs[None]), C.c_void_p(pw or 0),
                                               C.c_void_p(int(stream or 0))), L=self.L)
        return out

    def bake_probe_volume(self, origin, spacing, dims, depth_spp, max_distance, depth_seed=1, out=None, stream=None, indirect_only=False, **params):
        """mcpt_bake_probe_volume: bake_probe_grid, then query_probe_depth (depth_spp samples, max_distance, depth_seed) on the same
        scene-owned points -> (sh (probes, 27), moments (probes, 192), counts (probes, 2), Stats).  out: a dict with "sh", "moments" and
        "counts" device buffers; None: torch tensors on the scene's device.  indirect_only: as for query_probes (mcpt_bake_probe_volume_ex)."""
        who = "bake_probe_volume"
        g, m = _probe_grid(who, origin, spacing, dims)
        if m > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
            raise ValueError("%s: at most (2^31 - 1) / 192 probes, not %d" % (who, m))
        dp = _probe_depth_params(who, depth_spp, max_distance, depth_seed)
        spec = {"sh": ((m, 27), "float32"), "moments": ((m, PROBE_DEPTH_ROW), "float32"), "counts": ((m, 2), "int32")}
        out, ptrs, stream = _outputs(who, spec, out, self._torch_device() if out is None else None, stream)
        p = self.params(**params)
        st = Stats()
        _check(self.L.mcpt_bake_probe_volume_ex(self.h, C.byref(g), C.byref(p), C.byref(dp), C.c_void_p(ptrs["sh"]), C.c_void_p(ptrs["moments"]),
                                                C.c_void_p(ptrs["counts"]), C.c_void_p(int(stream or 0)), C.byref(st), _probe_opts(indirect_only)), L=self.L)
        return out["sh"], out["moments"], out["counts"], st

    def render_probe_lit(self, origin, spacing, dims, sh, moments=None, counts=None, normal_bias=0.0, backface_max=0.25, aov_spp=0, specular_depth=0,
                         centre=False, seed=1, camera=None, position=False, out=None, stream=None, direct_samples=0, direct_seed=1):
        """mcpt_render_probe_lit: a frame of the live scene lit by the probe volume (origin, spacing, dims, sh (probes, 27)) -> (lit (H, W, 3),
        position (H, W, 3) or None, mcpt_lit_info as a dict), float32 device buffers.  moments (probes, 192) and counts (probes, 2) together:
        the occlusion-aware lookup with (normal_bias, backface_max); both None: the plain one.  aov_spp (0: 1), specular_depth, centre, seed
        and camera as for render_aovs.  out: a dict with a "lit" device buffer (and "position" when position is asked); None: torch
        tensors on the scene's device.  Works on `stream` and blocks until the outputs are complete.  direct_samples > 0
        (mcpt_render_probe_lit_direct): that many light samples of the sampled direct term per surface sample, drawn with direct_seed, are
        added to the lookup; the dict then also holds light_samples, shadow_rays and pieces."""
        who = "render_probe_lit"
        if not 0 <= int(direct_samples) <= DIRECT_MAX_SAMPLES:
            raise ValueError("%s: direct_samples must be in 0 .. %d, not %r" % (who, DIRECT_MAX_SAMPLES, direct_samples))
        g, m = _probe_grid(who, origin, spacing, dims)
        if (moments is None) != (counts is None):
            raise ValueError("%s: moments and counts come together (both None: the plain lookup)" % who)
        o = _lit_opts(who, aov_spp, specular_depth, centre, seed)
        ps = _device_array(who, "sh", sh, (m, 27))
        pm = pc = 0
        vis = None
        if moments is not None:
            if m > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
                raise ValueError("%s: at most (2^31 - 1) / 192 probes, not %d" % (who, m))
            vis = _probe_visibility(who, normal_bias, backface_max)
            pm = _device_array(who, "moments", moments, (m, PROBE_DEPTH_ROW))
            pc = _device_array(who, "counts", counts, (m, 2), "int32")
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        if W <= 0 or H <= 0:
            raise ValueError("%s: the camera's width and height are positive, not %d x %d" % (who, W, H))
        names = ("lit", "position") if position else ("lit",)
        out, ptrs, stream = _outputs(who, {w: ((H, W, 3), "float32") for w in names}, out, self._torch_device() if out is None else None, stream)
        vol = ProbeVolume(C.pointer(g), ps or None, pm or None, pc or None, C.pointer(vis) if vis is not None else None)
        outs = LitOutputs(ptrs["lit"] or None, ptrs.get("position") or None, (C.c_void_p * 2)(None, None))
        info = LitInfo()
        if int(direct_samples) > 0:
            d, di = LitDirectOpts(n_samples=int(direct_samples), seed=int(direct_seed) & 0xffffffff), LitDirectInfo()
            _check(self.L.mcpt_render_probe_lit_direct(self.h, _ptr(cam), C.byref(o), C.byref(d), C.byref(vol), C.byref(outs), C.c_void_p(int(stream or 0)),
                                                       C.byref(info), C.byref(di)), L=self.L)
            return out["lit"], (out["position"] if position else None), dict(info.as_dict(), **di.as_dict())
        _check(self.L.mcpt_render_probe_lit(self.h, _ptr(cam), C.byref(o), C.byref(vol), C.byref(outs), C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return out["lit"], (out["position"] if position else None), info.as_dict()

    def relight_probe_volume(self, origin, spacing, dims, sh, moments=None, counts=None, normal_bias=0.0, backface_max=0.25, spp=64, seed=1, sample_offset=0,
                             hysteresis=0.0, indirect_only=False, direct_samples=0, direct_seed=1, depth=False, max_distance=None, out=None, stream=None):
        """mcpt_probe_volume_relight: one update of the probe volume (origin, spacing, dims, sh (probes, 27)) from itself -> (sh (probes, 27),
        moments (probes, 192) or None, counts (probes, 2) or None, mcpt_query_info as a dict), device buffers.  Every probe gathers spp
        whole-sphere rays (seed, sample_offset): a ray's hit is shaded from the previous volume -- moments and counts together: the
        occlusion-aware lookup with (normal_bias, backface_max); both None: the plain one -- plus direct_samples light samples drawn with
        direct_seed, and the fresh projection is blended with the previous coefficients: hysteresis is the share kept.  indirect_only: a
        ray that ends on an emitter records 0 (for a volume baked with indirect_only, together with direct_samples > 0).  depth: the depth
        maps of the same rays (max_distance required) come back as well.  out: a dict with an "sh" device buffer (and "moments", "counts"
        with depth) that must not overlap the inputs; None: torch tensors on the scene's device.  Enqueued on `stream` without a
        synchronisation, through the staging buffers of the ray queries; the inputs are not written."""
        who = "relight_probe_volume"
        g, m = _probe_grid(who, origin, spacing, dims)
        if (moments is None) != (counts is None):
            raise ValueError("%s: moments and counts come together (both None: the plain lookup)" % who)
        o = _probe_relight_opts(who, spp, seed, sample_offset, hysteresis, indirect_only, direct_samples, direct_seed, depth, max_distance)
        if m * o.spp > 2 ** 31 - 1 or m * o.spp * max(o.direct_samples, 1) > 2 ** 31 - 1:
            raise ValueError("%s: probes * spp and probes * spp * direct_samples must be at most 2^31 - 1" % who)
        ps = _device_array(who, "sh", sh, (m, 27))
        pm = pc = 0
        vis = None
        if (moments is not None or depth) and m > (2 ** 31 - 1) // PROBE_DEPTH_ROW:
            raise ValueError("%s: at most (2^31 - 1) / 192 probes, not %d" % (who, m))
        if moments is not None:
            vis = _probe_visibility(who, normal_bias, backface_max)
            pm = _device_array(who, "moments", moments, (m, PROBE_DEPTH_ROW))
            pc = _device_array(who, "counts", counts, (m, 2), "int32")
        spec = {"sh": ((m, 27), "float32")}
        if depth:
            spec.update({"moments": ((m, PROBE_DEPTH_ROW), "float32"), "counts": ((m, 2), "int32")})
        out, ptrs, stream = _outputs(who, spec, out, self._torch_device() if out is None else None, stream)
        vol = ProbeVolume(C.pointer(g), ps or None, pm or None, pc or None, C.pointer(vis) if vis is not None else None)
        outs = ProbeRelightOutputs(ptrs["sh"] or None, ptrs.get("moments") or None, ptrs.get("counts") or None, None)
        info = QueryInfo()
        _check(self.L.mcpt_probe_volume_relight(self.h, C.byref(vol), C.byref(o), C.byref(outs), C.c_void_p(int(stream or 0)), C.byref(info)), L=self.L)
        return out["sh"], (out["moments"] if depth else None), (out["counts"] if depth else None), info.as_dict()

    def probe_buffers(self):
        """mcpt_scene_probe_buffers -> (floats the scene-owned probe buffers hold, how often one of them was (re)allocated)."""
        f, a = C.c_int64(0), C.c_int64(0)
        _check(self.L.mcpt_scene_probe_buffers(self.h, C.byref(f), C.byref(a)), L=self.L)
        return int(f.value), int(a.value)

    def shadow_visible(self, origins, dirs, dist, found=None, shard=None, list=0):
        """mcpt_debug_shadow: the render loop's shadow query (k_trace_shadow, its retrace included) for rays of the caller's -> bool [n]:
        the closest hit of ray i lies within EPSILON of dist[i].  found[i] = 1 asserts that some primitive is hit within EPSILON of dist[i]
        (default: no assertion); shard[i] in 0..31 places ray i in the sharded queue (default: (i // 64) % 32); list: 0 or 1."""
        o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        ds = np.ascontiguousarray(dist, dtype=np.float32).reshape(-1)
        f = np.zeros(n, dtype=np.uint8) if found is None else np.ascontiguousarray(found, dtype=np.uint8).reshape(-1)
        sh = None if shard is None else np.ascontiguousarray(shard, dtype=np.int32).reshape(-1)
        if len(d) != n or len(ds) != n or len(f) != n or (sh is not None and len(sh) != n):
            raise ValueError("shadow_visible: the arrays do not describe %d rays" % n)
        vis = np.zeros(n, dtype=np.uint8)
        _check(self.L.mcpt_debug_shadow(self.h, int(list), n, _ptr(o), _ptr(d), _ptr(ds), _ptr(f), None if sh is None else _ptr(sh), _ptr(vis)),
               L=self.L)
        return vis.astype(bool)

    def classify(self, camera=None):
        """mcpt_debug_classify: the sky cull's classifier for every pixel -> (may_hit uint8 [H*W], cand int32 [H*W, 4], info dict); cand
        holds primitive ids in the order the walk found them, -1 unused, or -2 in column 0: the pixel's rays walk the tree."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        n = int(cam["width"].reshape(-1)[0]) * int(cam["height"].reshape(-1)[0])
        may_hit, cand = np.zeros(n, np.uint8), np.zeros((n, 4), np.int32)
        info = CullInfo()
        _check(self.L.mcpt_debug_classify(self.h, _ptr(cam), _ptr(may_hit), _ptr(cand), C.byref(info)), L=self.L)
        return may_hit, cand, info.as_dict()

    def cast_rays(self, origins, dirs, pixel, sample, channel, **kw):
        o = np.ascontiguousarray(origins, dtype=np.float32)
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        n = len(o)
        px = np.ascontiguousarray(pixel, dtype=np.uint32)
        sm = np.ascontiguousarray(sample, dtype=np.uint32)
        ch = np.ascontiguousarray(channel, dtype=np.int32)
        out = np.zeros(n, dtype=np.float32)
        p = self.params(**kw)
        _check(self.L.mcpt_cast_rays(self.h, C.byref(p), n, _ptr(o), _ptr(d), _ptr(px), _ptr(sm), _ptr(ch), _ptr(out)), L=self.L)
        return out

    def centre_rays(self, pixels, camera=None):
        """mcpt_centre_rays: the centre rays of `pixels` (m = j*W + i) -> (origins[n,3], dirs[n,3]) float32: through the pixel centre and
        the centre of the lens, a function of the camera alone."""
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        px = np.ascontiguousarray(pixels, dtype=np.uint32)
        n = len(px)
        o = np.zeros((n, 3), dtype=np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        _check(self.L.mcpt_centre_rays(self.h, _ptr(cam), n, _ptr(px), _ptr(o), _ptr(d)), L=self.L)
        return o, d

    def camera_rays(self, pixels, samples, seed=1, camera=None):
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        px = np.ascontiguousarray(pixels, dtype=np.uint32)
        sm = np.ascontiguousarray(samples, dtype=np.uint32)
        n = len(px)
        o = np.zeros((n, 3), dtype=np.float32)
        d = np.zeros((n, 3), dtype=np.float32)
        _check(self.L.mcpt_camera_rays(self.h, _ptr(cam), int(seed), n, _ptr(px), _ptr(sm), _ptr(o), _ptr(d)), L=self.L)
        return o, d


class HipSequence:
    """A frame sequence on a HipScene (mcpt_sequence_*): the history, its variance and every working buffer stay on the device.  The loop
    is `scene.update(...); seq.frame(seed=k)`."""

    _SHAPES = {"fb": (3,), "accumulated": (3,), "denoised": (3,), "variance": (), "len": (), "aov": (8,), "motion": (4,), "rgba": (4,)}

    def __init__(self, scene, width=None, height=None, filter=True, max_history=0, depth_tol=0.0, normal_test=False, color_clamp=False,
                 normal_min=0.0, clamp_k=0.0, history=None, adaptive=None, create_adaptive=False, specular_motion=False, motion=None,
                 weighted=None, moments=None, features=None, feedback=None, **denoise_opts_kw):
        """history: a HistoryOpts passed to mcpt_sequence_create_ex as it is (tests: a zeroed one must give mcpt_sequence_create's sequence).
        adaptive: a dict of sequence_adaptive's keywords or a SequenceAdaptive; create_adaptive: go through mcpt_sequence_create_adaptive
        even without one (tests: a null rule must give mcpt_sequence_create_ex's sequence).  specular_motion: mcpt_sequence_create_motion
        with the switch on; motion: a SequenceMotion passed to it as it is, or "null" for a null pointer (tests: a null or zeroed one must
        give mcpt_sequence_create_adaptive's sequence).  weighted: True for mcpt_sequence_create_weighted with the switch on; a
        SequenceWeighted passed to it as it is, or "null" for a null pointer (tests: a null or zeroed one must give
        mcpt_sequence_create_motion's sequence).  moments: True or a dict of moments_opts' keywords for mcpt_sequence_create_moments with
        the switch on; a MomentsOpts passed to it as it is, or "null" for a null pointer (tests: a null or zeroed one must give
        mcpt_sequence_create_weighted's sequence).  features: a FeatureOpts passed to mcpt_sequence_create_features as it is, or "null" for a
        null pointer (tests: a null or zeroed one must give mcpt_sequence_create_moments' sequence).  feedback: a FeedbackOpts passed to
        mcpt_sequence_create_feedback as it is, or "null" for a null pointer (tests: a null or zeroed one must give
        mcpt_sequence_create_features' sequence)."""
        self.scene = scene  # (keeps the scene alive as long as the sequence)
        self.L = scene.L
        self.h = None
        cam = scene.sd.camera
        self.W = int(width if width is not None else np.asarray(cam["width"]).reshape(-1)[0])
        self.H = int(height if height is not None else np.asarray(cam["height"]).reshape(-1)[0])
        o = SequenceOpts(temporal=temporal_opts(max_history, depth_tol), denoise=denoise_opts(**denoise_opts_kw), filter=int(bool(filter)))
        h = C.c_void_p()
        if history is None and (normal_test or color_clamp):
            history = history_opts(normal_test, color_clamp, normal_min, clamp_k)
        if isinstance(adaptive, dict):
            adaptive = sequence_adaptive(**adaptive)
        if specular_motion and motion is None:
            motion = SequenceMotion(specular_motion=1)
        if weighted is True:
            weighted = SequenceWeighted(weighted=1)
        if moments is True:
            moments = moments_opts()
        elif isinstance(moments, dict):
            moments = moments_opts(**moments)
        if feedback is not None:
            w = None if weighted is None or weighted is False or isinstance(weighted, str) else weighted
            m = None if moments is None or moments is False or isinstance(moments, str) else moments
            _check(self.L.mcpt_sequence_create_feedback(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                        None if adaptive is None else C.byref(adaptive),
                                                        None if motion is None or isinstance(motion, str) else C.byref(motion),
                                                        None if w is None else C.byref(w), None if m is None else C.byref(m),
                                                        None if features is None or isinstance(features, str) else C.byref(features),
                                                        None if isinstance(feedback, str) else C.byref(feedback), C.byref(h)), L=self.L)
        elif features is not None:
            w = None if weighted is None or weighted is False or isinstance(weighted, str) else weighted
            m = None if moments is None or moments is False or isinstance(moments, str) else moments
            _check(self.L.mcpt_sequence_create_features(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                        None if adaptive is None else C.byref(adaptive),
                                                        None if motion is None or isinstance(motion, str) else C.byref(motion),
                                                        None if w is None else C.byref(w), None if m is None else C.byref(m),
                                                        None if isinstance(features, str) else C.byref(features), C.byref(h)), L=self.L)
        elif moments is not None and moments is not False:
            w = None if weighted is None or weighted is False or isinstance(weighted, str) else weighted
            _check(self.L.mcpt_sequence_create_moments(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                       None if adaptive is None else C.byref(adaptive),
                                                       None if motion is None or isinstance(motion, str) else C.byref(motion),
                                                       None if w is None else C.byref(w),
                                                       None if isinstance(moments, str) else C.byref(moments), C.byref(h)), L=self.L)
        elif weighted is not None and weighted is not False:
            _check(self.L.mcpt_sequence_create_weighted(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                        None if adaptive is None else C.byref(adaptive),
                                                        None if motion is None or isinstance(motion, str) else C.byref(motion),
                                                        None if isinstance(weighted, str) else C.byref(weighted), C.byref(h)), L=self.L)
        elif motion is not None:
            _check(self.L.mcpt_sequence_create_motion(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                      None if adaptive is None else C.byref(adaptive),
                                                      None if isinstance(motion, str) else C.byref(motion), C.byref(h)), L=self.L)
        elif adaptive is not None or create_adaptive:
            _check(self.L.mcpt_sequence_create_adaptive(scene.h, self.W, self.H, C.byref(o), None if history is None else C.byref(history),
                                                        None if adaptive is None else C.byref(adaptive), C.byref(h)), L=self.L)
        elif history is None:
            _check(self.L.mcpt_sequence_create(scene.h, self.W, self.H, C.byref(o), C.byref(h)), L=self.L)
        else:
            _check(self.L.mcpt_sequence_create_ex(scene.h, self.W, self.H, C.byref(o), C.byref(history), C.byref(h)), L=self.L)
        self.h = h

    def frame(self, camera=None, want=("denoised",), **params_kw):
        """mcpt_sequence_frame: renders, accumulates and (filter) denoises one frame; vary `seed` from frame to frame.  want: the outputs to
        copy to the host, of SEQUENCE_OUTPUTS.  Returns a dict of those arrays ([H,W,c] float32; rgba uint8), "info" (stage times in ms,
        frame_index) and "stats"."""
        cam = np.ascontiguousarray(camera if camera is not None else self.scene.sd.camera)
        out, ptrs = {}, SequenceOutputs()
        for k in want:
            if k not in self._SHAPES:
                raise ValueError("unknown sequence output %r (one of %s)" % (k, ", ".join(SEQUENCE_OUTPUTS)))
            out[k] = np.empty((self.H, self.W) + self._SHAPES[k], dtype=np.uint8 if k == "rgba" else np.float32)
            setattr(ptrs, k, out[k].ctypes.data)
        p = self.scene.params(**params_kw)
        info, st = SequenceInfo(), Stats()
        _check(self.L.mcpt_sequence_frame(self.h, _ptr(cam), C.byref(p), C.byref(ptrs), C.byref(info), C.byref(st)), L=self.L)
        out["info"], out["stats"] = info.as_dict(), st
        return out

    def flags(self):
        """mcpt_sequence_flags: flags[H,W] uint8 of the last frame (FLAG_NORMAL | FLAG_CLAMP per pixel); a sequence without history
        rejection keeps none and raises."""
        out = np.zeros((self.H, self.W), dtype=np.uint8)
        _check(self.L.mcpt_sequence_flags(self.h, _ptr(out)), L=self.L)
        return out

    def weight(self):
        """mcpt_sequence_weight: weight[H,W] float32, the samples behind each pixel of the last frame's history (0 before the first frame); a
        sequence created without weighted keeps none and raises."""
        out = np.zeros((self.H, self.W), dtype=np.float32)
        _check(self.L.mcpt_sequence_weight(self.h, _ptr(out)), L=self.L)
        return out

    def moments(self):
        """mcpt_sequence_moments: moments[H,W,2] float32, the running first and second moment of each pixel's luminance after the last frame
        (0 before the first frame); a sequence created without moments keeps none and raises."""
        out = np.zeros((self.H, self.W, 2), dtype=np.float32)
        _check(self.L.mcpt_sequence_moments(self.h, _ptr(out)), L=self.L)
        return out

    def history(self, variance=True):
        """mcpt_sequence_history: (color[H,W,3], variance[H,W]) float32, the history the next frame will blend with: the fed planes of a
        feedback sequence, otherwise the accumulated colour and variance of the last frame (0 before the first).  variance=False passes a
        null variance pointer and returns (color, None); a moments sequence with feedback keeps no fed variance and raises for True."""
        color = np.zeros((self.H, self.W, 3), dtype=np.float32)
        var = np.zeros((self.H, self.W), dtype=np.float32) if variance else None
        _check(self.L.mcpt_sequence_history(self.h, _ptr(color), None if var is None else _ptr(var)), L=self.L)
        return color, var

    def counts(self):
        """mcpt_sequence_counts: dict(spp[H,W] int32, err[H,W], guide[H,W] float32 (0 without guided; the history weights of a weighted
        sequence), info dict) of the last frame of an
        adaptive sequence; any other sequence keeps none and raises."""
        spp = np.zeros((self.H, self.W), dtype=np.int32)
        err, guide = np.zeros((self.H, self.W), dtype=np.float32), np.zeros((self.H, self.W), dtype=np.float32)
        info = AdaptiveInfo()
        _check(self.L.mcpt_sequence_counts(self.h, _ptr(spp), _ptr(err), _ptr(guide), C.byref(info)), L=self.L)
        return dict(spp=spp, err=err, guide=guide, info=info.as_dict())

    def reset(self):
        """mcpt_sequence_reset, a camera cut: the next frame takes no history."""
        _check(self.L.mcpt_sequence_reset(self.h), L=self.L)

    def close(self):
        if getattr(self, "h", None):
            self.L.mcpt_sequence_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipGroup:
    """One replica of the scene per listed device; render() = mcpt_group_render (tile partition + RCCL merge inside the library)."""

    def __init__(self, sd, devices, library=None):
        self.sd = sd
        self._keep = []
        self.L = lib(library)
        d = _make_desc(sd, self._keep)
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        self.h = None
        rc = self.L.mcpt_group_create(C.byref(d), len(dev), _ptr(dev), C.byref(h))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mcpt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, moves):
        """mcpt_group_update: HipScene.update on every replica."""
        arr, n = _moves(moves)
        rc = self.L.mcpt_group_update(self.h, n, C.cast(arr, C.c_void_p))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))

    def deform(self, items):
        """mcpt_group_deform: HipScene.deform on every replica; host arrays only (the library refuses a device buffer: one pointer cannot
        be valid on several devices)."""
        arr, n, keep = _vertex_items(items, _mesh_tri_counts(self.sd))
        rc = self.L.mcpt_group_deform(self.h, n, C.cast(arr, C.c_void_p))
        del keep
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))

    def set_materials(self, edits=(), assign=()):
        """mcpt_group_set_materials: HipScene.set_materials on every replica."""
        ea, ne, aa, na = _material_lists(edits, assign)
        rc = self.L.mcpt_group_set_materials(self.h, ne, C.cast(ea, C.c_void_p), na, C.cast(aa, C.c_void_p))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))

    def set_environment(self, background, env=None):
        """mcpt_group_set_environment: HipScene.set_environment on every replica."""
        bg, w, h, px, keep = _environment(background, env)
        rc = self.L.mcpt_group_set_environment(self.h, C.cast(bg, C.c_void_p), w, h, px)
        del keep
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))

    def set_visibility(self, items):
        """mcpt_group_set_visibility: HipScene.set_visibility on every replica."""
        arr, n = _visibility_items(items)
        rc = self.L.mcpt_group_set_visibility(self.h, n, C.cast(arr, C.c_void_p))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))

    def add_objects(self, objects, triangles, materials=None):
        """mcpt_group_add_objects: HipScene.add_objects on every replica.  Returns (index of the first added object, {})."""
        a, arrays = _addition(self.sd, objects, triangles, materials)
        first = C.c_int32(-1)
        rc = self.L.mcpt_group_add_objects(self.h, C.byref(a), C.byref(first))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))
        self.sd = extend_scene(self.sd, *arrays)
        return int(first.value), {}

    def info(self):
        i = GroupInfo()
        rc = self.L.mcpt_group_get_info(self.h, C.byref(i))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))
        return {k: getattr(i, k) for k, _ in i._fields_}

    def render(self, camera=None, fb=None, **kw):
        cam = np.ascontiguousarray(camera if camera is not None else self.sd.camera)
        W, H = int(cam["width"].reshape(-1)[0]), int(cam["height"].reshape(-1)[0])
        if fb is None:
            fb = np.zeros((H, W, 3), dtype=np.float32)
        p = HipScene.params(self, **kw)
        st = Stats()
        rc = self.L.mcpt_group_render(self.h, _ptr(cam), C.byref(p), _ptr(fb), C.byref(st))
        if rc != 0:
            raise McptError(rc, self.L.mcpt_group_last_error().decode("utf-8", "replace"))
        return fb, st


_FMATH_SCENE = None


def debug_fmath(kind, x, y=None):
    """csrc/mcpt_fmath.h evaluated on the device (mcpt_debug_fmath): kind "sin" | "cos" | "atan2" | "acos"."""
    global _FMATH_SCENE
    if _FMATH_SCENE is None:
        from . import scenes
        _FMATH_SCENE = HipScene(scenes.cornell_rc(8, 8, 1))
    k = {"sin": 0, "cos": 1, "atan2": 2, "acos": 3, "pow": 4, "tonemap": 5}[kind]
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), dtype=np.float32)
    out = np.zeros_like(x)
    _check(lib().mcpt_debug_fmath(_FMATH_SCENE.h, k, x.size, _ptr(x), _ptr(y), _ptr(out)))
    return out
