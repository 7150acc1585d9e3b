"""Feature buffers behind mirrors and glass without a GPU (include/mcpt.h: mcpt_render_aovs_ex, mcpt_denoise_opts.specular_depth): the
options struct keeps its size with the new field at offset 20, out-of-range depths are refused by all three calls before any device call,
the remaining reserved words are still checked, and the header states the contract."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_options_layout(hip):
    assert C.sizeof(hip.DenoiseOpts) == 32
    assert hip.DenoiseOpts.specular_depth.offset == 20
    assert hip.DenoiseOpts.reserved.offset == 24 and hip.DenoiseOpts.reserved.size == 8
    assert hip.denoise_opts(specular_depth=4).specular_depth == 4
    assert hip.denoise_opts().specular_depth == 0
    assert "mcpt_render_aovs_ex" in hip.EXPORTS


def test_depth_out_of_range_is_refused_before_any_device_call(hip, pkg):
    L = hip.lib()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)  # (not a scene: the checks come first)
    W = H = 16
    cam = pkg.scenes.cornell_demo(W, H, 8).camera.copy()
    camp = cam.ctypes.data_as(C.c_void_p)
    buf = lambda n: C.cast((C.c_float * n)(), C.c_void_p)
    col, var, aov, out = buf(W * H * 3), buf(W * H), buf(W * H * 8), buf(W * H * 3)

    def render_denoised(o):
        p = hip.Params(spp=16, rr_rate=0.7, n_dir_sample=4, enable_shadow=1, seed=1, tile_size=32, nranks=1)
        return L.mcpt_render_denoised(fake, camp, C.byref(p), C.byref(o), col, out, None, None, None, None)

    for d in (-1, 9, 1 << 30, -(1 << 31)):
        o = hip.denoise_opts(specular_depth=d)
        assert L.mcpt_denoise(fake, W, H, col, var, aov, C.byref(o), out) == 1, d
        assert b"mcpt_denoise" in L.mcpt_last_error()
        assert render_denoised(o) == 1, d
        assert b"mcpt_render_denoised" in L.mcpt_last_error()
        assert L.mcpt_render_aovs_ex(fake, camp, 1, 4, d, aov) == 1, d
        assert b"mcpt_render_aovs_ex" in L.mcpt_last_error() and b"specular_depth" in L.mcpt_last_error()
    # the other checks of mcpt_render_aovs hold for the new call
    assert L.mcpt_render_aovs_ex(None, camp, 1, 4, 2, aov) == 1
    assert L.mcpt_render_aovs_ex(fake, None, 1, 4, 2, aov) == 1
    assert L.mcpt_render_aovs_ex(fake, camp, 1, 4, 2, None) == 1
    for n in (-1, 65537):
        assert L.mcpt_render_aovs_ex(fake, camp, 1, n, 2, aov) == 1, n
    cam0 = cam.copy()
    cam0["width"] = 0
    assert L.mcpt_render_aovs_ex(fake, cam0.ctypes.data_as(C.c_void_p), 1, 4, 2, aov) == 1


def test_reserved_words_are_still_refused(hip, pkg):
    L = hip.lib()
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)
    W = H = 8
    buf = lambda n: C.cast((C.c_float * n)(), C.c_void_p)
    col, var, aov, out = buf(W * H * 3), buf(W * H), buf(W * H * 8), buf(W * H * 3)
    for k in (0, 1):
        o = hip.denoise_opts(specular_depth=4)
        o.reserved[k] = 1
        assert L.mcpt_denoise(fake, W, H, col, var, aov, C.byref(o), out) == 1, k
    # the word the old reserved[1] occupied (offset 24): refused through the raw bytes as well
    raw = (C.c_int32 * 8)(0, 0, 0, 0, 0, 0, 1, 0)
    assert L.mcpt_denoise(fake, W, H, col, var, aov, C.byref(hip.DenoiseOpts.from_buffer(raw)), out) == 1


def test_header_documents_the_contract():
    h = open(os.path.join(ROOT, "include", "mcpt.h")).read()
    assert "} mcpt_denoise_opts;     /* 32 bytes */" in h
    assert re.search(r"int32_t specular_depth;", h) and re.search(r"int32_t reserved\[2\];", h)
    assert "int mcpt_render_aovs_ex(mcpt_scene *scene, const mcpt_camera *camera, uint32_t seed, int32_t aov_spp, int32_t specular_depth, float *aov_host);" in h
    i = h.index("Feature samples that see through mirrors and glass")
    c = h[i:h.index("int mcpt_render_aovs_ex(")]
    steps = [c.index(s) for s in ("1. trace the closest hit", "2. a miss", "3. a hit", "4. if b < specular_depth", "5. otherwise the sample records")]
    assert steps == sorted(steps)
    for text in ("channel 1", "kr > 0.5", "thr = (1,1,1)", "tsum += t", "depth = (float) tsum", "specular_depth 0 gives exactly mcpt_render_aovs",
                 "outside 0..8"):
        assert text in c, text
    assert "mcpt_render_aovs_ex(params.seed, opts.aov_spp, opts.specular_depth)" in h
