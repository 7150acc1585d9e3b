"""Every live edit in turn on ONE handle (include/mcpt.h: mcpt_scene_update, _deform, _set_visibility, _add_objects, _set_materials,
_set_environment): after each step the frame equals, bit for bit, the frame of a scene freshly created from the description the steps so
far amount to, and mcpt_update_info reports the path and the triangle count written below.  The per-edit tests pin the edits pairwise; this
one pins what each of them leaves behind for all the others.

The scene is cornell_demo without its short box and its plastic sphere (those two come back in step 4), 32 x 32 at 2 samples per pixel and
one seed.  The fresh description is composed with the library's own host rules: transform_triangles and deform_triangles
(deform_cases.deformed_scene), extend_scene's restatement (add_cases.extend_numpy) and compact_scene."""
import dataclasses
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import material_edit_cases as mc  # noqa: E402
from add_cases import extend_numpy, split  # noqa: E402
from deform_cases import DEVICE_BUILDERS, deformed_scene, object_positions, rotate_y, same_bits, translate, wave  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
W = H = 32
SPP = 2
SEED = 5
# the kept description, in Scene::Add order without the two objects that are added later; materials keep cornell_demo's indices
FLOOR, TALL, LEFT, RIGHT, LIGHT, GLASS_SPHERE, MIRROR_SPHERE = range(7)
BOX, BALL = 7, 8  # the added short box and plastic sphere
NEW_MAT = 9       # the material that arrives with them
BACKGROUND = (0.1, 0.1, 0.2)
# per step: (path on lbvh / ploc, n_moved_tris); on sah the path is 0 wherever it is 1 here
EXPECTED = [(1, 10), (1, 10), (1, 2), (1, 10), (2, 10), (0, 0), (1, 2), (1, 10), (2, 0)]


@dataclasses.dataclass
class Chain:
    """What the steps so far amount to: the base description, the latest positions and transforms given, the mask, the sky."""
    sd: object
    bases: dict = dataclasses.field(default_factory=dict)
    moves: dict = dataclasses.field(default_factory=dict)
    hidden: set = dataclasses.field(default_factory=set)
    sky: dict = dataclasses.field(default_factory=dict)

    def description(self, pkg, hip):
        now = deformed_scene(pkg, hip, self.sd, self.bases, self.moves)
        if self.hidden:
            mask = np.ones(len(now.objects), bool)
            mask[list(self.hidden)] = False
            now, _ = hip.compact_scene(now, mask)
        return dataclasses.replace(now, **self.sky)


def steps_of(pkg, hip):
    """The nine steps: (name, call on a HipScene or HipGroup, the same edit on the Chain)."""
    s = pkg.scenes
    cornell = s.cornell_demo(W, H, SPP)
    kept, (objs, tris) = split(hip, cornell, [mc.SHORT, mc.PLASTIC_SPHERE])
    assert len(kept.materials) == NEW_MAT and [int(kept.objects["n_tri"][o]) for o in (TALL, LEFT)] == [10, 2] and len(tris) == 10
    objs["material"][0] = NEW_MAT
    green = s._mat(s.ROUGH_CONDUCTOR, 0.2, (0.2, 0.9, 0.3))
    turn = rotate_y(0.3, (368, 165, 351), shift=(-20, 0, -30))
    bent = wave(object_positions(kept, TALL), amp=8.0)
    M = kept.materials
    swap = [(mc.TALL, mc.with_fields(M[mc.TALL], emission=(5, 6, 7))), (mc.LIGHT, mc.with_fields(M[mc.LIGHT], emission=(0, 0, 0)))]
    assert int(kept.objects["material"][TALL]) == mc.TALL and int(kept.objects["material"][LIGHT]) == mc.LIGHT
    env = mc.env_map(16, 8, 1)
    shift = translate(25, 10, -15)

    def extend(c):
        c.sd = extend_numpy(c.sd, objs, tris, [green])

    def reassign(c):
        c.sd = mc.edited_scene(c.sd, [], [(BOX, mc.RIGHT)])

    def relight(c):
        c.sd = mc.edited_scene(c.sd, swap, [])

    steps = [
        ("update", lambda h: h.update([(TALL, turn)]), lambda c: c.moves.update({TALL: turn})),
        ("deform", lambda h: h.deform([(TALL, bent)]), lambda c: c.bases.update({TALL: bent})),
        ("hide", lambda h: h.set_visibility([(LEFT, False)]), lambda c: c.hidden.add(LEFT)),
        ("add", lambda h: h.add_objects(objs, tris, [green])[1], extend),
        ("material in place", lambda h: h.set_materials(assign=[(BOX, mc.RIGHT)]), reassign),
        ("emitters swapped", lambda h: h.set_materials(swap), relight),
        ("show", lambda h: h.set_visibility([(LEFT, True)]), lambda c: c.hidden.discard(LEFT)),
        ("update the added mesh", lambda h: h.update([(BOX, shift)]), lambda c: c.moves.update({BOX: shift})),
        ("environment", lambda h: h.set_environment(BACKGROUND, env), lambda c: c.sky.update(background=np.asarray(BACKGROUND, f32), env_pixels=env)),
    ]
    assert len(steps) == len(EXPECTED)
    return kept, steps


@pytest.mark.parametrize("builder", ["sah", "lbvh", "ploc"])
def test_every_edit_in_turn_equals_a_fresh_scene(pkg, hip, builder):
    kept, steps = steps_of(pkg, hip)
    hs = hip.HipScene(kept, builder=builder)
    chain = Chain(kept)
    last = hs.render(spp=SPP, seed=SEED)[0]
    for (name, call, record), (path, n_tris) in zip(steps, EXPECTED):
        info = call(hs)
        record(chain)
        want_path = 0 if path == 1 and builder not in DEVICE_BUILDERS else path
        print(builder, name, "path", info["path"], "n_moved_tris", info["n_moved_tris"])
        assert info["path"] == want_path and info["n_moved_tris"] == n_tris, (name, info)
        fresh = hip.HipScene(chain.description(pkg, hip), builder=builder)
        a, b = hs.render(spp=SPP, seed=SEED)[0], fresh.render(spp=SPP, seed=SEED)[0]
        fresh.close()
        differing = int((~same_bits(a, b)).sum())
        print(builder, name, "differing floats", differing)
        assert differing == 0, (name, differing)
        assert not same_bits(a, last).all(), name  # (and every step shows)
        last = a
    hs.close()


@pytest.mark.parametrize("builder", ["sah", "ploc"])
def test_a_group_takes_the_same_steps(pkg, hip, monkeypatch, builder):
    """Two replicas on one device: after every step mcpt_group_render equals the frame of a single scene that took the same steps (which the
    test above holds against a fresh scene).  mcpt_group_create takes no build options, so the builder comes from MCPT_BVH, for the group and
    for the single scene alike: the host path throughout under sah, the device path wherever EXPECTED says 1 under ploc; the single scene's
    mcpt_update_info shows which one was taken."""
    monkeypatch.setenv("MCPT_BVH", builder)
    kept, steps = steps_of(pkg, hip)
    hs, g = hip.HipScene(kept), hip.HipGroup(kept, [0, 0])
    for (name, call, _), (path, _) in zip(steps, EXPECTED):
        info = call(hs)
        assert info["path"] == (0 if path == 1 and builder not in DEVICE_BUILDERS else path), (name, info)
        call(g)
        a, b = g.render(spp=SPP, seed=SEED)[0], hs.render(spp=SPP, seed=SEED)[0]
        assert same_bits(a, b).all(), name
    g.close()
    hs.close()
