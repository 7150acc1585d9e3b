"""Shared by tests/test_scene_visibility_cpu.py and tests/test_gpu_scene_visibility.py: masks, the numpy restatement of
mcpt_compact_scene, and the translation of primitive ids through prim_map."""
import numpy as np

f32 = np.float32
# cornell_demo, Scene::Add order: floor, short box, tall box, left, right, light, glass sphere, plastic sphere, mirror sphere
FLOOR, SHORT, TALL, LEFT, RIGHT, LIGHT, GLASS_SPHERE, PLASTIC_SPHERE, MIRROR_SPHERE = range(9)


def mask_hiding(sd, hidden):
    m = np.ones(len(sd.objects), bool)
    m[list(hidden)] = False
    return m


def masks_for(sd):
    """name -> mask: first object hidden, last hidden, two adjacent meshes hidden, every sphere hidden, every mesh but one hidden."""
    kind = sd.objects["kind"]
    meshes, spheres = np.flatnonzero(kind == 0), np.flatnonzero(kind == 1)
    adjacent = next((a, b) for a, b in zip(meshes[:-1], meshes[1:]) if b == a + 1 and a > 0)
    keep_one = meshes[len(meshes) // 2]
    return {"first": mask_hiding(sd, [0]), "last": mask_hiding(sd, [len(kind) - 1]), "adjacent": mask_hiding(sd, adjacent),
            "spheres": mask_hiding(sd, spheres), "one_mesh": mask_hiding(sd, [m for m in meshes if m != keep_one])}


def live_ids(sd, ob):
    """The primitive ids of object `ob` in a scene of `sd`."""
    o = sd.objects[ob]
    if o["kind"] == 0:
        return np.arange(int(o["first_tri"]), int(o["first_tri"]) + int(o["n_tri"]), dtype=np.int64)
    return np.array([len(sd.triangles) + ob], np.int64)


def compact_numpy(sd, mask):
    """mcpt_compact_scene restated: (objects, triangles, prim_map).  Triangles of the visible meshes in array order."""
    objs, nt = sd.objects, len(sd.triangles)
    prim_map = np.full(nt + len(objs), -1, np.int32)
    keep_tri = np.zeros(nt, bool)
    for ob in np.flatnonzero(mask):
        if objs["kind"][ob] == 0:
            keep_tri[live_ids(sd, ob)] = True
    prim_map[:nt][keep_tri] = np.arange(int(keep_tri.sum()), dtype=np.int32)
    out = objs[mask].copy()
    for k, ob in enumerate(np.flatnonzero(mask)):
        if objs["kind"][ob] == 0:
            out["first_tri"][k] = prim_map[int(objs["first_tri"][ob])]
        else:
            prim_map[nt + ob] = int(keep_tri.sum()) + k
    return out, sd.triangles[keep_tri].copy(), prim_map


def translate_ids(prim, prim_map):
    """Live primitive ids (-1: no hit) as the ids of the compacted description; a hidden id becomes -2, which no fresh scene reports."""
    prim = np.asarray(prim)
    out = np.where(prim >= 0, prim_map[np.maximum(prim, 0)], prim)
    return np.where((prim >= 0) & (out < 0), -2, out).astype(prim.dtype)


def translate_children(children, prim_map):
    """The child references of a tree dump with every leaf ~p replaced by ~prim_map[p]."""
    c = np.asarray(children).copy()
    leaf = c < 0
    c[leaf] = ~translate_ids(~c[leaf], prim_map)
    return c
