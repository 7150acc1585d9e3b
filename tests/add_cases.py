"""Shared by tests/test_scene_add_cpu.py and tests/test_gpu_scene_add.py (include/mcpt.h: mcpt_extend_scene, mcpt_scene_add_objects):
the numpy restatement of mcpt_extend_scene, the split of a description into "kept" plus "addition", and the reordered description
"kept objects, then added ones" that a scene must equal after the addition."""
import dataclasses

import numpy as np

f32 = np.float32


def extend_numpy(sd, objects, triangles, materials=None):
    """mcpt_extend_scene restated: objects after the existing ones in the order given, their first_tri shifted by the old triangle count;
    triangles and materials appended; everything else untouched."""
    obj = np.array(objects, dtype=sd.objects.dtype).reshape(-1)
    obj["first_tri"][obj["kind"] == 0] += len(sd.triangles)
    tri = np.zeros(0, sd.triangles.dtype) if triangles is None else np.asarray(triangles, dtype=sd.triangles.dtype).reshape(-1)
    mat = np.zeros(0, sd.materials.dtype) if materials is None else np.array(materials, dtype=sd.materials.dtype).reshape(-1)
    return dataclasses.replace(sd, objects=np.concatenate([sd.objects, obj]), triangles=np.concatenate([sd.triangles, tri]),
                               materials=np.concatenate([sd.materials, mat]))


def addition_of(sd, added):
    """(objects, triangles) that add the objects `added` of sd, in that order: their triangles packed in that order, first_tri relative to
    the packed array."""
    objs, tris, at = sd.objects[list(added)].copy(), [], 0
    for k, ob in enumerate(added):
        if sd.objects["kind"][ob] == 0:
            a, n = int(sd.objects["first_tri"][ob]), int(sd.objects["n_tri"][ob])
            tris.append(sd.triangles[a:a + n])
            objs["first_tri"][k] = at
            at += n
    return objs, (np.concatenate(tris) if tris else np.zeros(0, sd.triangles.dtype))


def split(hip, sd, added):
    """kept (the description without the objects `added`: mcpt_compact_scene), and the addition that brings them back."""
    mask = np.ones(len(sd.objects), bool)
    mask[list(added)] = False
    kept, _ = hip.compact_scene(sd, mask)
    return kept, addition_of(sd, added)


def reordered(hip, sd, added):
    """sd with the objects `added` moved behind the others: what a scene of `kept` equals after they have been added."""
    kept, (objs, tris) = split(hip, sd, added)
    return extend_numpy(kept, objs, tris)


def same_description(a, b):
    return a.objects.tobytes() == b.objects.tobytes() and a.triangles.tobytes() == b.triangles.tobytes() and a.materials.tobytes() == b.materials.tobytes()


def ids_of(sd, ob):
    """The primitive ids of object `ob` in a scene of `sd`."""
    o = sd.objects[ob]
    if o["kind"] == 0:
        return np.arange(int(o["first_tri"]), int(o["first_tri"]) + int(o["n_tri"]), dtype=np.int64)
    return np.array([len(sd.triangles) + ob], np.int64)
