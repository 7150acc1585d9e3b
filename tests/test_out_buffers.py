"""Every HipScene method that takes out=, without a GPU: the checks of the output buffers (a missing name, another element type, another
shape, a row stride, no out at all with inputs that are not torch tensors) raise ValueError before the library is called, and a correct
set of buffers reaches the library entry with every address in its argument slot.  The buffers are fake objects that only expose
__cuda_array_interface__ (FakeDevice of tests/ray_query_cases.py), each over an address of its own; the library is a recorder."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ray_query_cases import FakeDevice  # noqa: E402

N, W, H = 5, 8, 4                                     # items of a query, the size of a map or frame
GRID = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2, 1, 2))  # origin, spacing, dims of a probe grid
M = 4                                                 # its probes
STREAM = 0x7700
F4, F8, I4, U1 = "<f4", "<f8", "<i4", "|u1"
ITEM = {F4: 4, F8: 8, I4: 4, U1: 1}


class Recorder:
    """Stands for the library: every entry records (name, arguments) and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class FakeScene:
    """HipScene's methods over a recording library and a handle that is never used."""

    def __init__(self, hip):
        self.hip, self.h, self.L, self.device = hip, None, Recorder(), 0
        self.sd = type("sd", (), {})()
        self.sd.camera = np.zeros(1, dtype=[("width", np.int32), ("height", np.int32)])
        self.sd.camera["width"], self.sd.camera["height"] = W, H

    def __getattr__(self, name):
        return getattr(self.hip.HipScene, name).__get__(self)

    def params(self, **kw):
        return self.hip.Params(spp=1, rr_rate=0.8, n_dir_sample=1, nranks=1)


def val(a):
    """The address an argument carries: a c_void_p's, or an integer."""
    return int(getattr(a, "value", a) or 0)


def fields(a, *names):
    """The addresses in the members `names` of the structure passed by reference."""
    return {w: int(getattr(a._obj, w) or 0) for w in names}


# method -> (inputs {name: (shape, typestr)}, outputs {name: (shape, typestr)} ("out": a bare buffer), whether out=None is an error
# without torch inputs, call(scene, inputs, out, stream), the library entry, slots(args) -> {name: address as the library sees it})
RAYS = {"origins": ((N, 3), F4), "dirs": ((N, 3), F4), "tmax": ((N,), F4)}
VOLUME = {"sh": ((M, 27), F4), "moments": ((M, 192), F4), "counts": ((M, 2), I4)}
POINTS = {"points": ((N, 3), F4), "normals": ((N, 3), F4)}
HITS = {"t": ((N,), F8), "prim": ((N,), I4), "object": ((N,), I4), "uv": ((N, 2), F4), "normal": ((N, 3), F4), "point": ((N, 3), F4)}
TEXELS = {"texel": ((W * H,), I4), "prim": ((W * H,), I4), "bary": ((W * H, 2), F4), "origins": ((W * H, 3), F4), "normals": ((W * H, 3), F4)}
PLANES = {"image": ((H, W, 3), F4), "coverage": ((H, W), U1), "variance": ((H, W, 3), F4)}
LIT = {"lit": ((H, W, 3), F4), "position": ((H, W, 3), F4)}


def lit_slots(vol, outs, stream):
    return lambda a: dict(fields(a[vol], "sh", "moments", "counts"), **fields(a[outs], "lit", "position"), stream=val(a[stream]))


CASES = {
    "query_closest": (RAYS, HITS, True,
                      lambda hs, i, out, s: hs.query_closest(i["origins"], i["dirs"], i["tmax"], want=tuple(HITS), out=out, stream=s),
                      "mcpt_query_closest", lambda a: dict(fields(a[2], *RAYS), **fields(a[3], *HITS), stream=val(a[4]))),
    "query_occluded": (RAYS, {"out": ((N,), U1)}, True,
                       lambda hs, i, out, s: hs.query_occluded(i["origins"], i["dirs"], i["tmax"], out=out, stream=s),
                       "mcpt_query_occluded", lambda a: dict(fields(a[2], *RAYS), out=val(a[3]), stream=val(a[4]))),
    "query_radiance": ({k: RAYS[k] for k in ("origins", "dirs")}, {"radiance": ((N, 3), F4), "variance": ((N, 3), F4)}, True,
                       lambda hs, i, out, s: hs.query_radiance(i["origins"], i["dirs"], variance=True, out=out, stream=s),
                       "mcpt_query_radiance", lambda a: dict(fields(a[3], "origins", "dirs"), **fields(a[4], "radiance", "variance"), stream=val(a[5]))),
    "lightmap_texels": ({}, TEXELS, False,
                        lambda hs, i, out, s: hs.lightmap_texels(1, W, H, out=out, stream=s),
                        "mcpt_lightmap_texels", lambda a: dict(fields(a[2], *TEXELS), stream=val(a[4]))),
    "lightmap_scatter": ({"texel": ((N,), I4), "values": ((N, 3), F4)}, {k: PLANES[k] for k in ("image", "coverage")}, False,
                         lambda hs, i, out, s: hs.lightmap_scatter(0, W, H, i["texel"], i["values"], out=out, stream=s),
                         "mcpt_lightmap_scatter", lambda a: dict(texel=val(a[3]), values=val(a[4]), image=val(a[6]), coverage=val(a[7]), stream=val(a[8]))),
    "bake_lightmap": ({}, PLANES, False,
                      lambda hs, i, out, s: hs.bake_lightmap(0, W, H, variance=True, out=out, stream=s),
                      "mcpt_bake_lightmap", lambda a: dict(image=val(a[4]), coverage=val(a[5]), variance=val(a[6]), stream=val(a[7]))),
    "query_probes": ({"origins": ((N, 3), F4)}, {"sh": ((N, 27), F4), "radiance": ((N, 3), F4), "variance": ((N, 3), F4)}, True,
                     lambda hs, i, out, s: hs.query_probes(i["origins"], variance=True, out=out, stream=s),
                     "mcpt_query_probes_ex", lambda a: dict(fields(a[4], "sh", "radiance", "variance"), origins=val(a[3]), stream=val(a[5]))),
    "probe_shade": (dict(POINTS, sh=VOLUME["sh"]), {"out": ((N, 3), F4)}, True,
                    lambda hs, i, out, s: hs.probe_shade(*GRID, i["sh"], i["points"], i["normals"], out=out, stream=s),
                    "mcpt_probe_shade", lambda a: dict(sh=val(a[2]), points=val(a[4]), normals=val(a[5]), out=val(a[6]), stream=val(a[7]))),
    "bake_probe_grid": ({}, {"out": ((M, 27), F4)}, False,
                        lambda hs, i, out, s: hs.bake_probe_grid(*GRID, out=out, stream=s),
                        "mcpt_bake_probe_grid_ex", lambda a: dict(out=val(a[3]), stream=val(a[4]))),
    "query_probe_depth": ({"origins": ((N, 3), F4)}, {"moments": ((N, 192), F4), "counts": ((N, 2), I4)}, True,
                          lambda hs, i, out, s: hs.query_probe_depth(i["origins"], 4, 1.0, out=out, stream=s),
                          "mcpt_query_probe_depth", lambda a: dict(origins=val(a[3]), moments=val(a[4]), counts=val(a[5]), stream=val(a[6]))),
    "query_direct": (POINTS, {"out": ((N, 3), F4)}, True,
                     lambda hs, i, out, s: hs.query_direct(i["points"], i["normals"], 2, out=out, stream=s),
                     "mcpt_query_direct", lambda a: dict(points=val(a[3]), normals=val(a[4]), out=val(a[5]), stream=val(a[6]))),
    "probe_shade_visible": (dict(POINTS, weight=((N,), F4), **VOLUME), {"out": ((N, 3), F4)}, True,
                            lambda hs, i, out, s: hs.probe_shade_visible(*GRID, i["sh"], i["moments"], i["counts"], i["points"], i["normals"],
                                                                         weight=i["weight"], out=out, stream=s),
                            "mcpt_probe_shade_visible",
                            lambda a: dict(sh=val(a[2]), moments=val(a[3]), counts=val(a[4]), points=val(a[7]), normals=val(a[8]), out=val(a[9]),
                                           weight=val(a[10]), stream=val(a[11]))),
    "bake_probe_volume": ({}, VOLUME, False,
                          lambda hs, i, out, s: hs.bake_probe_volume(*GRID, 4, 1.0, out=out, stream=s),
                          "mcpt_bake_probe_volume_ex", lambda a: dict(sh=val(a[4]), moments=val(a[5]), counts=val(a[6]), stream=val(a[7]))),
    "render_probe_lit": (VOLUME, LIT, False,
                         lambda hs, i, out, s: hs.render_probe_lit(*GRID, i["sh"], i["moments"], i["counts"], position=True, out=out, stream=s),
                         "mcpt_render_probe_lit", lit_slots(3, 4, 5)),
    "render_probe_lit, direct": (VOLUME, LIT, False,
                                 lambda hs, i, out, s: hs.render_probe_lit(*GRID, i["sh"], i["moments"], i["counts"], position=True, out=out, stream=s,
                                                                           direct_samples=2),
                                 "mcpt_render_probe_lit_direct", lit_slots(4, 5, 6)),
}


def buffers(spec, first):
    """FakeDevice buffers for a spec, each over an address of its own -> ({name: buffer}, {name: address})."""
    addr = {w: first + 0x1000 * k for k, w in enumerate(spec)}
    return {w: FakeDevice(shape, ts, ptr=addr[w]) for w, (shape, ts) in spec.items()}, addr


def as_out(outputs, bufs):
    return bufs["out"] if tuple(outputs) == ("out",) else dict(bufs)


def row_strided(shape, ts):
    """The strides of an array of `shape` whose rows lie twice as far apart as they are long."""
    strides, acc = [], ITEM[ts]
    for d in reversed(shape):
        strides.insert(0, acc)
        acc *= d
    strides[0] *= 2
    return tuple(strides)


@pytest.mark.parametrize("method", sorted(CASES))
def test_good_buffers_reach_the_library_in_their_slots(hip, method):
    inputs, outputs, _, call, entry, slots = CASES[method]
    hs = FakeScene(hip)
    ins, in_addr = buffers(inputs, 0x100000)
    outs, out_addr = buffers(outputs, 0x900000)
    call(hs, ins, as_out(outputs, outs), STREAM)
    assert [name for name, _ in hs.L.calls] == [entry]
    assert slots(hs.L.calls[0][1]) == dict(in_addr, **out_addr, stream=STREAM)


@pytest.mark.parametrize("method", sorted(CASES))
def test_bad_outputs_raise_before_the_library(hip, method):
    inputs, outputs, needs_out, call, _, _ = CASES[method]
    hs = FakeScene(hip)
    ins, _ = buffers(inputs, 0x100000)
    good, _ = buffers(outputs, 0x900000)
    for w, (shape, ts) in outputs.items():
        bad = {"another element type": FakeDevice(shape, F8 if ts == F4 else F4),
               "another shape": FakeDevice((shape[0] + 1,) + shape[1:], ts),
               "flattened": FakeDevice((int(np.prod(shape)), 1), ts),
               "a row stride": FakeDevice(shape, ts, strides=row_strided(shape, ts)),
               "a host array": np.zeros(shape, np.float32)}
        for what, b in bad.items():
            with pytest.raises(ValueError):
                call(hs, ins, as_out(outputs, dict(good, **{w: b})), STREAM)
            assert not hs.L.calls, (w, what)
        if w != "out":
            with pytest.raises(ValueError):
                call(hs, ins, {k: v for k, v in good.items() if k != w}, STREAM)
            assert not hs.L.calls, w
    if needs_out:
        with pytest.raises(ValueError):
            call(hs, ins, None, STREAM)
        assert not hs.L.calls


def test_probe_calls_pass_their_options_only_when_asked(hip):
    """The three probe calls go through their _ex entry once: a null options pointer is the plain call (include/mcpt.h)."""
    for method, slot in (("query_probes", 7), ("bake_probe_grid", 6), ("bake_probe_volume", 9)):
        inputs, outputs, _, _, entry, _ = CASES[method]
        for flag in (False, True):
            hs = FakeScene(hip)
            ins, _ = buffers(inputs, 0x100000)
            outs, _ = buffers(outputs, 0x900000)
            args = ((ins["origins"],) if method == "query_probes" else GRID) + ((4, 1.0) if method == "bake_probe_volume" else ())
            getattr(hs, method)(*args, out=as_out(outputs, outs), indirect_only=flag)
            (name, a), = hs.L.calls
            assert name == entry and len(a) == slot + 1
            assert (a[slot]._obj.indirect_only == 1) if flag else (a[slot] is None)


def test_accumulate_needs_the_callers_buffers(hip):
    hs = FakeScene(hip)
    with pytest.raises(ValueError):
        hs.query_probe_depth(FakeDevice((N, 3)), 4, 1.0, accumulate=1)
    assert not hs.L.calls
