"""mcpt_query_closest / mcpt_query_occluded without a GPU: the struct sizes of include/mcpt.h, the null-scene refusal, and the shape, dtype
and contiguity checks of HipScene.query_closest / query_occluded, which raise before the library is called (the buffers here are fake
objects that only expose __cuda_array_interface__)."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402


def test_struct_sizes(hip):
    assert C.sizeof(hip.RayBuffers) == 24
    assert C.sizeof(hip.HitBuffers) == 48
    assert C.sizeof(hip.QueryInfo) == 32


def test_null_scene_is_refused(hip):
    L = hip.lib()
    rays, hits, info = hip.RayBuffers(), hip.HitBuffers(), hip.QueryInfo()
    assert L.mcpt_query_closest(None, 1, C.byref(rays), C.byref(hits), None, C.byref(info)) == 1
    assert b"mcpt_query_closest: null scene" in L.mcpt_last_error()
    assert L.mcpt_query_occluded(None, 1, C.byref(rays), None, None, None) == 1
    assert b"mcpt_query_occluded: null scene" in L.mcpt_last_error()
    assert L.mcpt_query_closest(None, 0, None, None, None, None) == 1


class NoLibraryScene:
    """HipScene's query methods over a handle that must never be used: every case below is refused before the library is called."""

    def __init__(self, hip):
        self.h, self.L = None, None
        self.query_closest = hip.HipScene.query_closest.__get__(self)
        self.query_occluded = hip.HipScene.query_occluded.__get__(self)


GOOD = dict(origins=lambda n: FakeDevice((n, 3)), dirs=lambda n: FakeDevice((n, 3)), tmax=lambda n: FakeDevice((n,)))
BAD_RAYS = {
    "origins float64": dict(origins=lambda n: FakeDevice((n, 3), "<f8")),
    "dirs int32": dict(dirs=lambda n: FakeDevice((n, 3), "<i4")),
    "origins flat": dict(origins=lambda n: FakeDevice((n * 3,))),
    "origins (n, 4)": dict(origins=lambda n: FakeDevice((n, 4))),
    "dirs of another length": dict(dirs=lambda n: FakeDevice((n + 1, 3))),
    "origins transposed": dict(origins=lambda n: FakeDevice((n, 3), strides=(4, 4 * n))),
    "dirs with a row stride": dict(dirs=lambda n: FakeDevice((n, 3), strides=(16, 4))),
    "tmax (n, 1)": dict(tmax=lambda n: FakeDevice((n, 1))),
    "tmax float64": dict(tmax=lambda n: FakeDevice((n,), "<f8")),
    "tmax strided": dict(tmax=lambda n: FakeDevice((n,), strides=(8,))),
    "origins a host list": dict(origins=lambda n: [[0.0, 0.0, 0.0]] * n),
}


@pytest.mark.parametrize("case", sorted(BAD_RAYS))
def test_bad_rays_raise_before_the_library(hip, case):
    n = 8
    args = {k: (BAD_RAYS[case].get(k) or GOOD[k])(n) for k in GOOD}
    hs = NoLibraryScene(hip)
    out = {"t": FakeDevice((n,), "<f8"), "prim": FakeDevice((n,), "<i4")}
    with pytest.raises(ValueError):
        hs.query_closest(args["origins"], args["dirs"], args["tmax"], out=out)
    with pytest.raises(ValueError):
        hs.query_occluded(args["origins"], args["dirs"], args["tmax"], out=FakeDevice((n,), "|u1"))


def test_bad_outputs_raise_before_the_library(hip):
    n = 8
    hs = NoLibraryScene(hip)
    o, d, tm = FakeDevice((n, 3)), FakeDevice((n, 3)), FakeDevice((n,))
    with pytest.raises(ValueError):  # no torch tensors: the outputs must be supplied
        hs.query_closest(o, d)
    with pytest.raises(ValueError):
        hs.query_occluded(o, d, tm)
    with pytest.raises(ValueError):  # tmax is required for occlusion
        hs.query_occluded(o, d, None, out=FakeDevice((n,), "|u1"))
    with pytest.raises(ValueError):  # an unknown output, none at all, a repeated one
        hs.query_closest(o, d, want=("t", "depth"), out={})
    with pytest.raises(ValueError):
        hs.query_closest(o, d, want=(), out={})
    with pytest.raises(ValueError):
        hs.query_closest(o, d, want=("t", "t"), out={"t": FakeDevice((n,), "<f8")})
    with pytest.raises(ValueError):  # a wanted output without a buffer
        hs.query_closest(o, d, want=("t", "prim"), out={"t": FakeDevice((n,), "<f8")})
    for name, bad in (("t", FakeDevice((n,), "<f4")), ("prim", FakeDevice((n,), "<f4")), ("object", FakeDevice((n, 1), "<i4")),
                      ("uv", FakeDevice((n, 3))), ("normal", FakeDevice((n * 3,))), ("point", FakeDevice((n, 3), strides=(4, 4 * n))),
                      ("uv", FakeDevice((n - 1, 2)))):
        with pytest.raises(ValueError):
            hs.query_closest(o, d, want=(name,), out={name: bad})
    with pytest.raises(ValueError):
        hs.query_occluded(o, d, tm, out=FakeDevice((n,), "<i4"))
    with pytest.raises(ValueError):
        hs.query_occluded(o, d, tm, out=FakeDevice((n + 1,), "|u1"))


def test_device_positions_still_checked(hip):
    """The shape check of HipScene.deform now shares its helper with the queries: its own refusals stay."""
    assert hip._device_positions(FakeDevice((4, 3, 3))).n_tri == 4
    assert hip._device_positions(FakeDevice((36,))).n_tri == 4
    for bad in (FakeDevice((4, 3, 3), "<f8"), FakeDevice((4, 3, 3), strides=(36, 4, 12)), FakeDevice((4, 9)), FakeDevice((35,))):
        with pytest.raises(ValueError):
            hip._device_positions(bad)
    assert hip._device_positions([1.0, 2.0]) is None
