"""Shared by tests/test_scene_materials_cpu.py and tests/test_gpu_scene_materials.py (include/mcpt.h: mcpt_scene_set_materials,
mcpt_scene_set_environment): the description desc' an edited scene must equal, the numpy restatement of the device's material record,
of the emission predicate that selects the path and of the segment table of k_set_materials, the edits the GPU tests apply, and a
generated environment map.  The comparison rules are those of tests/deform_cases.py.  No tests in here."""
import dataclasses

import numpy as np

f32 = np.float32
K_EPS = f32(1e-4)  # EPSILON, csrc/mcpt_internal.h
MAT_EMISSIVE, MAT_TEXTURED = 0x80000000, 0x40000000
# MaterialRec, csrc/mcpt_internal.h (96 bytes)
REC_DTYPE = np.dtype([("type", np.int32), ("textured", np.int32), ("isDirac", np.int32), ("hasEmission", np.int32),
                      ("roughness", f32), ("iorA", f32), ("iorB", f32), ("pad0", f32), ("refl", f32, 3), ("pad1", f32),
                      ("emit", f32, 3), ("pad2", f32), ("ior", f32, 3), ("pad3", f32), ("inv_ior", f32, 3), ("pad4", f32)])
# MatSeg, csrc/mcpt_material.h (32 bytes)
SEG_DTYPE = np.dtype([("first_lane", np.int32), ("count", np.int32), ("first_tri", np.int32), ("object", np.int32),
                      ("mat_bits", np.uint32), ("mat", np.int32), ("pad", np.int32, 2)])
assert REC_DTYPE.itemsize == 96 and SEG_DTYPE.itemsize == 32
# cornell_demo: Scene::Add order and, one material per object, the material table's order
FLOOR, SHORT, TALL, LEFT, RIGHT, LIGHT, GLASS_SPHERE, PLASTIC_SPHERE, MIRROR_SPHERE = range(9)


# ---------------------------------------------------------------- restatements
def emits(mats):
    """Material::hasEmission in float32: sqrtf(e.e) > EPSILON with the 3-term dot order x*x + (y*y + z*z)."""
    e = np.asarray(mats["emission"], f32).reshape(-1, 3)
    with np.errstate(over="ignore"):
        z = e[:, 0] * e[:, 0] + (e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        assert z.dtype == f32
        return np.sqrt(z) > K_EPS


def material_records(mats):
    """mat::make_record restated: every operation in float32 in the stated order, the reciprocal through a double division."""
    mats = np.atleast_1d(mats)
    r = np.zeros(len(mats), REC_DTYPE)
    r["type"], r["textured"] = mats["type"], (mats["textured"] != 0)
    r["isDirac"] = (mats["type"] == 0) | (mats["type"] == 2)
    r["hasEmission"] = emits(mats)
    for k in ("roughness", "iorA", "iorB"):
        r[k] = mats[k]
    r["refl"], r["emit"] = mats["base_reflectance"], mats["emission"]
    wl = np.array([0.700, 0.5461, 0.4358], f32)
    with np.errstate(all="ignore"):
        ior = mats["iorA"].astype(f32)[:, None] + mats["iorB"].astype(f32)[:, None] / (wl * wl)[None, :]
        assert ior.dtype == f32
        r["ior"] = ior
        r["inv_ior"] = (1.0 / ior.astype(np.float64)).astype(f32)
    return r


def object_emits(sd):
    return emits(sd.materials)[sd.objects["material"]]


def edited_scene(sd, edits=(), assign=(), **replace):
    """desc': the listed material entries replaced, the listed objects reassigned; replace: background= / env_pixels= of the description."""
    mats, objs = sd.materials.copy(), sd.objects.copy()
    for i, m in edits:
        mats[i] = m
    for o, m in assign:
        objs["material"][o] = m
    return dataclasses.replace(sd, materials=mats, objects=objs, **replace)


def predicted_path(sd, edits=(), assign=()):
    """2 (in place) when every object emits after the call iff it did before, else 0 (host)."""
    return 2 if np.array_equal(object_emits(sd), object_emits(edited_scene(sd, edits, assign))) else 0


def predicted_segments(sd, edits=(), assign=()):
    """The segment table of k_set_materials: in object order, every object listed in `assign` and every mesh whose material changes its
    `textured` flag; a mesh takes one lane per triangle, a sphere one."""
    after = edited_scene(sd, edits, assign)
    listed = {int(o) for o, _ in assign}
    em = emits(after.materials)
    segs, lane = [], 0
    for o in range(len(sd.objects)):
        was, now = sd.objects[o], after.objects[o]
        mesh = int(now["kind"]) == 0
        tex0, tex1 = int(sd.materials["textured"][was["material"]]) != 0, int(after.materials["textured"][now["material"]]) != 0
        if not (o in listed or (mesh and tex0 != tex1)):
            continue
        m = int(now["material"])
        bits = m | (MAT_EMISSIVE if em[m] else 0) | (MAT_TEXTURED if (mesh and tex1) else 0)
        count = int(now["n_tri"]) if mesh else 1
        segs.append((lane, count, int(now["first_tri"]) if mesh else -1, o, bits, m))
        lane += count
    out = np.zeros(len(segs), SEG_DTYPE)
    for k, s in enumerate(segs):
        out[k] = s + ((0, 0),)
    return out


def patched_triangles(sd, edits=(), assign=()):
    """info.n_moved_tris on path 2: the triangle records among the segments' lanes."""
    s = predicted_segments(sd, edits, assign)
    return int(s["count"][s["first_tri"] >= 0].sum())


def with_fields(m, **kw):
    """A copy of the material record m with fields replaced."""
    src, m = m, np.zeros((), dtype=m.dtype)  # (np.array(record, copy=True) still shares the record's memory)
    for k in m.dtype.names:
        m[k] = src[k]
    for k, v in kw.items():
        m[k] = v
    return m


def env_map(w, h, seed=0):
    """A generated (h, w, 3) map in [0, 1]: a vertical gradient times a few coloured lobes, different for every seed and size."""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid((np.arange(h) + 0.5) / h, (np.arange(w) + 0.5) / w, indexing="ij")
    ph = rng.uniform(0, 6.28, 3)
    img = np.stack([0.5 + 0.5 * np.sin(6.28 * u * (k + 1) + ph[k]) * (1 - v) for k in range(3)], -1)
    return np.ascontiguousarray(np.clip(0.15 + 0.8 * img, 0, 1), dtype=f32)


# ---------------------------------------------------------------- the in-place edits of the GPU tests
def cornell_steps(pkg, sd, zoo):
    """(name, edits, assign) in order, each applied to the scene the previous ones left.  `zoo`: (materials, names) of
    material_zoo.zoo_materials().  Works on cornell_demo and on cornell_rc (which has no spheres: their step is left out)."""
    s = pkg.scenes
    M = sd.materials
    zm, zn = zoo
    light = int(np.flatnonzero(emits(M))[0])
    has_spheres = bool((sd.objects["kind"] == 1).any())
    short_mat = int(sd.objects["material"][SHORT])
    left_mat = int(sd.objects["material"][LEFT])
    steps = [
        ("recolour", [(left_mat, with_fields(M[left_mat], base_reflectance=(0.2, 0.3, 0.9), roughness=0.35))], []),
        ("rough to smooth conductor", [(short_mat, with_fields(M[short_mat], type=s.SMOOTH_CONDUCTOR, roughness=0.001))], []),
        ("smooth conductor to glass", [(short_mat, zm[zn.index("type2_rough0.01_ior2.4+0.45_textured")])], []),
        ("glass from outside the presets, untextured", [(short_mat, with_fields(zm[zn.index("type2_rough0_ior0.75+0")], textured=0))], []),
        ("textured floor", [(int(sd.objects["material"][FLOOR]), with_fields(M[sd.objects["material"][FLOOR]], textured=1))], []),
        ("piece reassigned", [], [(TALL, short_mat)]),
    ]
    if has_spheres:
        steps.append(("sphere reassigned", [], [(PLASTIC_SPHERE, int(sd.objects["material"][MIRROR_SPHERE]))]))
    steps.append(("light dimmed", [(light, with_fields(M[light], emission=(M[light]["emission"] * f32(0.25)).astype(f32)))], []))
    return steps
