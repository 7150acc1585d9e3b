"""mcpt_query_radiance / mcpt_sensor_rays without a GPU: the struct sizes of include/mcpt.h, the null-scene refusal, and the shape, dtype
and contiguity checks of HipScene.query_radiance, which raise before the library is called (the buffers here are fake objects that only
expose __cuda_array_interface__)."""
import ctypes as C
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402


def test_struct_sizes(hip):
    assert C.sizeof(hip.SensorBuffers) == 32
    assert C.sizeof(hip.SensorOutputs) == 16
    assert hip.SENSOR_KINDS == {"ray": 0, "hemisphere": 1}


def test_null_scene_is_refused(hip):
    L = hip.lib()
    p, sensors, outs, st = hip.Params(spp=1, rr_rate=0.8, n_dir_sample=1, nranks=1), hip.SensorBuffers(), hip.SensorOutputs(), hip.Stats()
    assert L.mcpt_query_radiance(None, C.byref(p), 1, C.byref(sensors), C.byref(outs), None, C.byref(st)) == 1
    assert b"mcpt_query_radiance: null scene" in L.mcpt_last_error()
    assert L.mcpt_query_radiance(None, None, 0, None, None, None, None) == 1
    assert b"mcpt_query_radiance" in L.mcpt_last_error()
    assert L.mcpt_sensor_rays(None, 0, 1, 0, None, None, None, None, None, None) == 1
    assert b"mcpt_sensor_rays" in L.mcpt_last_error()


class NoLibraryScene:
    """HipScene.query_radiance over a handle that must never be used: every case below is refused before the library is called."""

    def __init__(self, hip):
        self.h, self.L, self.sd = None, None, None
        self.query_radiance = hip.HipScene.query_radiance.__get__(self)

    def params(self, **kw):
        raise AssertionError("the parameters were built: the inputs passed their checks")


GOOD = dict(origins=lambda n: FakeDevice((n, 3)), dirs=lambda n: FakeDevice((n, 3)))
BAD_SENSORS = {
    "origins float64": dict(origins=lambda n: FakeDevice((n, 3), "<f8")),
    "dirs int32": dict(dirs=lambda n: FakeDevice((n, 3), "<i4")),
    "origins flat": dict(origins=lambda n: FakeDevice((n * 3,))),
    "origins (n, 4)": dict(origins=lambda n: FakeDevice((n, 4))),
    "dirs of another length": dict(dirs=lambda n: FakeDevice((n + 1, 3))),
    "origins transposed": dict(origins=lambda n: FakeDevice((n, 3), strides=(4, 4 * n))),
    "dirs with a row stride": dict(dirs=lambda n: FakeDevice((n, 3), strides=(16, 4))),
    "origins a host list": dict(origins=lambda n: [[0.0, 0.0, 0.0]] * n),
    "dirs a host list": dict(dirs=lambda n: [[0.0, 0.0, 1.0]] * n),
}


@pytest.mark.parametrize("case", sorted(BAD_SENSORS))
def test_bad_sensors_raise_before_the_library(hip, case):
    n = 8
    args = {k: (BAD_SENSORS[case].get(k) or GOOD[k])(n) for k in GOOD}
    hs = NoLibraryScene(hip)
    for kind in ("ray", "hemisphere"):
        with pytest.raises(ValueError):
            hs.query_radiance(args["origins"], args["dirs"], kind=kind, out={"radiance": FakeDevice((n, 3))})


def test_bad_kind_and_outputs_raise_before_the_library(hip):
    n = 8
    hs = NoLibraryScene(hip)
    o, d = FakeDevice((n, 3)), FakeDevice((n, 3))
    good = {"radiance": FakeDevice((n, 3)), "variance": FakeDevice((n, 3))}
    for kind in ("sphere", 1, None, "RAY"):
        with pytest.raises(ValueError):
            hs.query_radiance(o, d, kind=kind, out=good)
    with pytest.raises(ValueError):  # no torch tensors: the outputs must be supplied
        hs.query_radiance(o, d)
    with pytest.raises(ValueError):  # a wanted output without a buffer
        hs.query_radiance(o, d, variance=True, out={"radiance": FakeDevice((n, 3))})
    for bad in (FakeDevice((n, 3), "<f8"), FakeDevice((n * 3,)), FakeDevice((n - 1, 3)), FakeDevice((n, 3), strides=(4, 4 * n)), [[0.0] * 3] * n):
        with pytest.raises(ValueError):
            hs.query_radiance(o, d, out={"radiance": bad})
        with pytest.raises(ValueError):
            hs.query_radiance(o, d, variance=True, out={"radiance": FakeDevice((n, 3)), "variance": bad})
    with pytest.raises(AssertionError):  # and good inputs do get as far as the parameters
        hs.query_radiance(o, d, variance=True, out=good)
