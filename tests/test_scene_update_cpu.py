"""Moving objects, the part that needs no GPU (include/mcpt.h: mcpt_scene_update, mcpt_transform_triangles).

mcpt_transform_triangles is the host build of csrc/mcpt_move.h, the header the scene builder and the update kernel compile as well: it
must equal a numpy float32 restatement of the point rule bit for bit,
    p'[r] = (m[4r]*p.x + (m[4r+1]*p.y + m[4r+2]*p.z)) + m[4r+3],
for any finite matrix, in place too, and copy the texture coordinates.  The argument checks of mcpt_scene_update that come before the
scene is looked at are reachable here and must refuse with MCPT_ERR_ARG."""
import ctypes as C

import numpy as np
import pytest

f32 = np.float32


def _matrices():
    c, s = f32(np.cos(0.7)), f32(np.sin(0.7))
    return {
        "identity": np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32),
        "translation": np.array([[1, 0, 0, 12.5], [0, 1, 0, -3.25], [0, 0, 1, 1e3]], f32),
        "rotation": np.array([[c, 0, s, 0.1], [0, 1, 0, 0.2], [-s, 0, c, 0.3]], f32),
        "scale": np.array([[2.5, 0, 0, 0], [0, 0.3, 0, 0], [0, 0, 7, 0]], f32),
        "reflection": np.array([[-1, 0, 0, 556], [0, 1, 0, 0], [0, 0, 1, 0]], f32),
        "zero_row": np.array([[0.3, -1.7, 0.9, 4], [0, 0, 0, 0], [1.1, 0.2, -0.6, -2]], f32),
    }


def _restated(m, p):
    """The point rule on an [n, 3] float32 array: every operation rounds to float32, in the stated order."""
    m = m.astype(f32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    for r in range(3):
        inner = (m[r, 1] * y).astype(f32) + (m[r, 2] * z).astype(f32)
        out[:, r] = ((m[r, 0] * x).astype(f32) + inner.astype(f32)).astype(f32) + m[r, 3]
    return out.astype(f32)


@pytest.fixture(scope="module")
def triangles(pkg):
    rng = np.random.default_rng(17)
    t = np.zeros(10000, pkg.scenes.TRI_DTYPE)
    for name in ("v0", "v1", "v2"):
        t[name] = (rng.normal(0, 1, (10000, 3)) * 10.0 ** rng.uniform(-3, 3, (10000, 1))).astype(f32)
    t["v0"][:8] = [[0, 0, 0], [-0.0, -0.0, -0.0], [1, 0, -0.0], [0, -0.0, 1], [-1, -1, -1], [1e-30, 0, 0], [3e38, 1, 1], [0, 1e-40, 0]]
    for name in ("t0", "t1", "t2"):
        t[name] = rng.uniform(-2, 2, (10000, 2)).astype(f32)
    return t


@pytest.mark.parametrize("name", list(_matrices()))
def test_transform_equals_the_restated_rule_bit_for_bit(hip, triangles, name):
    m = _matrices()[name]
    with np.errstate(over="ignore"):
        out = hip.transform_triangles(m, triangles)
        for v in ("v0", "v1", "v2"):
            want = _restated(m, triangles[v])
            assert np.array_equal(out[v].view(np.uint32), want.view(np.uint32)), (name, v, int((out[v].view(np.uint32) != want.view(np.uint32)).sum()))
    for t in ("t0", "t1", "t2"):
        assert np.array_equal(out[t].view(np.uint32), triangles[t].view(np.uint32))
    # in place
    again = triangles.copy()
    assert hip.transform_triangles(m, again, out=again) is again
    assert again.tobytes() == out.tobytes()


def test_identity_is_not_a_copy(hip, triangles):
    """Why an object that never got a transform is left alone instead of being multiplied by an identity: -0 + 0 = +0."""
    out = hip.transform_triangles(_matrices()["identity"], triangles)
    assert out["v0"][1].view(np.uint32).tolist() == [0, 0, 0] and triangles["v0"][1].view(np.uint32).tolist() == [0x80000000] * 3


def test_transform_argument_checks(hip, triangles):
    L = hip.lib()
    m = np.ascontiguousarray(_matrices()["rotation"])
    one = triangles[:1].copy()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.mcpt_transform_triangles(None, 1, p(one), p(one)) == 1
    assert L.mcpt_transform_triangles(p(m), -1, p(one), p(one)) == 1
    assert L.mcpt_transform_triangles(p(m), 1, None, p(one)) == 1
    assert L.mcpt_transform_triangles(p(m), 1, p(one), None) == 1
    assert L.mcpt_transform_triangles(p(m), 0, None, None) == 0
    for bad in (np.nan, np.inf, -np.inf):
        mb = m.copy()
        mb[1, 2] = bad
        assert L.mcpt_transform_triangles(p(mb), 1, p(one), p(one)) == 1 and b"not finite" in L.mcpt_last_error()
    assert one.tobytes() == triangles[:1].tobytes()


def test_update_argument_checks_before_the_scene_is_looked_at(hip):
    """n < 0, null moves, a non-finite entry and a duplicate are refused before the scene is dereferenced; a null scene after them."""
    L = hip.lib()
    good = hip.ObjectTransform(object=0, m=(C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0))
    info = hip.UpdateInfo()
    assert L.mcpt_scene_update(None, 1, C.byref(good), C.byref(info)) == 1 and b"null scene" in L.mcpt_last_error()
    assert L.mcpt_scene_update(None, 0, None, None) == 1 and b"null scene" in L.mcpt_last_error()
    assert L.mcpt_scene_update(None, -1, C.byref(good), None) == 1 and b"n < 0" in L.mcpt_last_error()
    assert L.mcpt_scene_update(None, 2, None, None) == 1 and b"null moves" in L.mcpt_last_error()
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in (0, 7, 11):
            mv = hip.ObjectTransform(object=0, m=(C.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0))
            mv.m[k] = bad
            assert L.mcpt_scene_update(None, 1, C.byref(mv), None) == 1 and b"not finite" in L.mcpt_last_error()
    two = (hip.ObjectTransform * 2)(good, good)
    assert L.mcpt_scene_update(None, 2, two, None) == 1 and b"listed twice" in L.mcpt_last_error()
    assert L.mcpt_group_update(None, 1, C.byref(good)) == 1 and b"null group" in L.mcpt_group_last_error()


def test_struct_sizes(hip):
    assert C.sizeof(hip.ObjectTransform) == 52
    assert C.sizeof(hip.UpdateInfo) == 56
