"""Adaptive sampling (mcpt_render_adaptive) without a GPU: the ctypes structs match the header's sizes, the call refuses null and
invalid arguments before it touches a device, and include/mcpt.h states the contract the GPU tests check."""
import ctypes as C
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_sizes(hip):
    assert C.sizeof(hip.Adaptive) == 32
    assert C.sizeof(hip.AdaptiveInfo) == 264


def test_null_arguments_are_rejected(hip):
    L = hip.lib()
    assert L.mcpt_render_adaptive(None, None, None, None, None, None, None, None, None) == 1
    assert b"null" in L.mcpt_last_error()


def test_invalid_options_are_rejected_before_any_device_call(hip, pkg):
    """Every rule of the argument check returns MCPT_ERR_ARG; the scene handle is never dereferenced for them."""
    L = hip.lib()
    fake_scene = C.create_string_buffer(64)  # (not a scene: the checks come first)
    cam = pkg.scenes.cornell_demo(16, 16, 8).camera
    cam = cam.copy()
    fb = (C.c_float * (16 * 16 * 3))()

    def call(spp=64, min_spp=8, threshold=0.1, rel_floor=1e-3, dilate=1, **pk):
        p = hip.Params(spp=spp, rr_rate=0.7, n_dir_sample=4, enable_shadow=1, seed=1, tile_size=32, nranks=1)
        for k, v in pk.items():
            setattr(p, k, v)
        o = hip.Adaptive(min_spp=min_spp, dilate=dilate, threshold=threshold, rel_floor=rel_floor)
        return L.mcpt_render_adaptive(C.cast(fake_scene, C.c_void_p), cam.ctypes.data_as(C.c_void_p), C.byref(p), C.byref(o), C.cast(fb, C.c_void_p),
                                      None, None, None, None)

    bad = [dict(spp=48), dict(spp=8 << 16), dict(min_spp=1, spp=64), dict(min_spp=0), dict(min_spp=-8), dict(threshold=-0.1),
           dict(threshold=float("inf")), dict(threshold=float("nan")), dict(rel_floor=0.0), dict(rel_floor=-1.0), dict(rel_floor=float("nan")),
           dict(dilate=2), dict(dilate=-1), dict(accumulate=1), dict(spp_total=64), dict(sample_offset=8)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert b"mcpt_render_adaptive" in L.mcpt_last_error(), kw


def test_header_documents_the_contract():
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    for text in ("mcpt_render_adaptive", "min_spp", "S0 * 2^R, 0 <= R <= 15", "m = s1[c]/n;  q = s2[c]/n - m*m;  var = max(q, 0) * n / (n - 1)",
                 "e_c = sqrt(var / n) / (m + rel_floor)", "2n <= params.spp", "BIT-IDENTICAL TO THE SAME PIXEL OF mcpt_render",
                 "} mcpt_adaptive; /* 32 bytes */", "} mcpt_adaptive_info; /* 264 bytes */", "MCPT_ERR_OVERFLOW"):
        assert text in h, text
