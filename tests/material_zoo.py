"""Materials outside the nine presets of scenes.material_presets(), and scenes that show them: what mcpt_scene_create accepts (any type
0..3 with any finite roughness, index of refraction, texture flag and emission) rather than what the shipped scenes use.  A helper for
tests/test_gpu_material.py and tests/test_gpu_material_zoo.py; no tests in here."""
import numpy as np

f32 = np.float32

ROUGHNESS = (0.0, 1e-4, 0.01, 0.2, 0.5, 1.0)
# (iorA, iorB): ior = A + B / lambda^2 per channel.  Index-matched, almost, water, glass, below one, diamond-like, blue 4.77, 5 and 6.
IORS = ((1.0, 0.0), (1.0001, 0.0), (1.33, 0.004), (1.5, 0.01), (0.75, 0.0), (2.4, 0.15), (2.4, 0.45), (5.0, 0.0), (6.0, 0.0))
REFLECTANCE = ((0.9, 0.6, 0.3), (0.2, 0.7, 0.4), (0.972, 0.960, 0.915))
# The two materials on either side of Material::hasEmission's threshold sqrtf(e.e) > 1e-4: norms 0.9e-4 and 1.1e-4
_E = np.array([2.0, 1.0, 2.0]) / 3.0


def _pkg():
    import mcpt_loader
    return mcpt_loader.load()


def zoo_materials():
    """(MAT_DTYPE array of 38 materials, their names).  Per type, nine materials: every (iorA, iorB) once, the six roughness values in
    turn (so each occurs with each type), both texture flags, and (5, 6, 7) of emission on one.  Then a rough conductor and a smooth
    dielectric whose emission straddles the hasEmission threshold."""
    s = _pkg().scenes
    mats, names = [], []
    for t in (s.SMOOTH_CONDUCTOR, s.ROUGH_CONDUCTOR, s.SMOOTH_DIELECTRIC, s.ROUGH_DIELECTRIC):
        for i, (a, b) in enumerate(IORS):
            rough = ROUGHNESS[(i + t) % len(ROUGHNESS)]
            tex = (i // 2 + t) % 2
            emit = (5.0, 6.0, 7.0) if i == (2 * t + 1) % len(IORS) else (0.0, 0.0, 0.0)
            mats.append(s._mat(t, rough, REFLECTANCE[(i + t) % 3], iorA=a, iorB=b, emission=emit, textured=tex))
            names.append("type%d_rough%g_ior%g+%g%s%s" % (t, rough, a, b, "_textured" if tex else "", "_emissive" if emit[0] else ""))
    mats.append(s._mat(s.ROUGH_CONDUCTOR, 0.2, REFLECTANCE[0], emission=tuple(0.9e-4 * _E)))
    names.append("type1_emission_below_threshold")
    mats.append(s._mat(s.SMOOTH_DIELECTRIC, 0.01, iorA=1.5, iorB=0.01, emission=tuple(1.1e-4 * _E)))
    names.append("type2_emission_above_threshold")
    assert len(set(names)) == len(names)
    return np.stack(mats).astype(s.MAT_DTYPE), names


def channel_ior(mat):
    """Material::ior per channel in float32 (Material.hpp:178-183: A + B / lambda^2, lambda = 0.700, 0.5461, 0.4358 micrometres,
    WaveLen.hpp:7-18), with the library's expression.  Tests compare functions of it bit for bit; here it only serves to BUILD inputs."""
    wl = np.array([0.700, 0.5461, 0.4358], f32)
    return (f32(mat["iorA"]) + f32(mat["iorB"]) / (wl * wl)).astype(f32)


def _quad(s, a, b, c, d):
    """Two triangles with texture coordinates that span the checkerboard's cells (u 0.3 ... 0.7, v 0 ... 0.7)."""
    t = np.zeros(2, s.TRI_DTYPE)
    t["v0"], t["v1"], t["v2"] = [a, a], [b, c], [c, d]
    t["t0"], t["t1"], t["t2"] = [(0.3, 0.0)] * 2, [(0.7, 0.0), (0.7, 0.7)], [(0.7, 0.7), (0.3, 0.7)]
    return t


def zoo_scene(materials, names, w, h, spp=4, name="zoo"):
    """A wall of objects above a rough floor under one quad emitter, one object per listed material in a grid facing the camera: a sphere,
    or -- for every textured material and every third of the others -- a slab of two faces, the front one facing the camera and the back
    one facing away, so that a path that passes the front meets the back from inside.  Returns (scene, material index of every object)."""
    s = _pkg().scenes
    P = s.material_presets()
    b = s._Builder()
    n = len(materials)
    cols = int(np.ceil(np.sqrt(1.5 * n)))
    rows = int(np.ceil(n / cols))
    pitch = 1.2
    b.add_mesh(_quad(s, (-12, -0.2, -12), (-12, -0.2, 12), (12, -0.2, 12), (12, -0.2, -12)), b.material("floor", P["rough_white_conductor"]))
    cx, top = 0.5 * (cols - 1) * pitch, rows * pitch
    b.add_mesh(_quad(s, (cx - 1.5, top + 1.5, 2.0), (cx + 1.5, top + 1.5, 2.0), (cx + 1.5, top + 1.5, 5.0), (cx - 1.5, top + 1.5, 5.0)),
               b.material("light", s._mat(s.ROUGH_CONDUCTOR, emission=(40, 35, 30))))
    for k in range(n):
        x, y = (k % cols) * pitch, 0.6 + (k // cols) * pitch
        mid = b.material(names[k], materials[k])
        if int(materials[k]["textured"]) or k % 3 == 0:
            e = 0.45
            front = _quad(s, (x - e, y - e, 0.25), (x + e, y - e, 0.15), (x + e, y + e, 0.15), (x - e, y + e, 0.25))
            back = _quad(s, (x - e, y - e, -0.15), (x - e, y + e, -0.15), (x + e, y + e, -0.25), (x + e, y - e, -0.25))
            b.add_mesh(np.concatenate([front, back]), mid)
        else:
            b.add_sphere((x, y, 0.0), 0.45, mid)
    height = rows * pitch + 0.4
    dist = max(0.5 * height, 0.5 * (cols * pitch + 0.2) * h / w) / np.tan(np.deg2rad(14.0))
    cam = s.make_camera(w, h, 28.0, (cx, 0.5 * height, dist), (cx, 0.5 * height, 0.0))
    sd = b.finish(background=np.float32([0.05, 0.05, 0.08]), camera=cam, rr_rate=0.8, spp=spp, name=name)
    return sd, [int(o["material"]) for o in sd.objects]


# The small cut: with the floor and the emitter exactly 12 materials (kSmallMats), 3 emitters (kSmallLights = 4; an emissive sphere
# and an emissive slab among them), 36 triangles: the LDS-resident flavour.  Every type, roughness 0 and 1, the indices 1, 0.75,
# 4.77 (blue) and 6, both texture flags.
SMALL_CUT = ("type0_rough0_ior1+0", "type0_rough0.01_ior1.33+0.004_textured", "type1_rough1_ior0.75+0_textured", "type2_rough0_ior0.75+0",
             "type2_rough0.01_ior2.4+0.45_textured", "type2_rough0.5_ior6+0", "type3_rough0_ior1.5+0.01", "type3_rough1_ior6+0_textured",
             "type2_rough0.0001_ior2.4+0.15_emissive", "type1_rough0.5_ior1.5+0.01_emissive")


def zoo_scene_small(w=96, h=64, spp=4):
    mats, names = zoo_materials()
    pick = [names.index(k) for k in SMALL_CUT]
    return zoo_scene(mats[pick], [names[k] for k in pick], w, h, spp, "zoo_small")


def zoo_scene_full(w=96, h=64, spp=4):
    mats, names = zoo_materials()
    return zoo_scene(mats, names, w, h, spp, "zoo_full")


# --------------------------------------------------------------------------- rows for mcpt_debug_material built from a material's own index
ROWS_PER_MATERIAL = 256
_COS_EDGE = float(np.cos(np.arccos(1.0 - 1e-4)))  # h.N on Material::eval's Dirac threshold 1 - EPSILON


def _ulps(x, j):
    """float32 x moved by j units in the last place."""
    x = f32(x)
    for _ in range(abs(j)):
        x = np.nextafter(x, f32(np.inf if j > 0 else -np.inf), dtype=f32)
    return x


def _frame(rng):
    n = rng.normal(size=3)
    n /= np.linalg.norm(n)
    t = np.cross(n, rng.normal(size=3))
    t /= np.linalg.norm(t)
    return n, t


def _tilted(rng, n, k):
    """A half vector whose cosine with n sits on 1 - EPSILON (k = -8 ... 8: about k float32 ulps of the cosine off it); k = None: n."""
    if k is None:
        return n
    t = np.cross(n, rng.normal(size=3))
    t /= np.linalg.norm(t)
    c = _COS_EDGE + 6e-8 * k
    return c * n + np.sqrt(1.0 - c * c) * t


def zoo_rows(rng, mat):
    """(rows [256, 13], channel [256], is_reflect [256]) for mcpt_debug_material, built from the material's per-channel index.  Rows are
    {a, b, c, uv, u1, u2}: eval / pdf read (wi, wo, N) = (a, b, c), fresnel / refract / reflect (I, N) = (a, b), sample N = a.
       0 ..  95  the critical angle of mat_fresnel (sint = 1) and mat_refract (k = 0), on the side of the surface that has one (cosi > 0
                 for an index above one, cosi < 0 below): 48 rows beyond it by 1 % ... 100 % of its cosine, 30 short of it, 9 within +-4
                 ulps of its cosine (N = z, so that I.N is I's z exactly), 9 the same seen from the other side;
      96 .. 127  Dirac refraction: wo the Snell image of wi about a half vector that is N (15 rows) or lies on h.N = 1 - EPSILON +- ulps;
     128 .. 159  Dirac reflection: the same with wo the mirror image of wi;
     160 .. 191  wi.n and wo.n out of {+0, -0, 1e-7, -1e-7}, with both values of is_reflect;
     192 .. 255  wi = wo = n with uv on the checkerboard's cell edges 0.05 + k / 10 and k / 12, their float neighbours, and inside cells."""
    ior3 = channel_ior(mat).astype(np.float64)
    rows = np.zeros((ROWS_PER_MATERIAL, 13), f32)
    ch = (np.arange(ROWS_PER_MATERIAL) % 3).astype(np.int32)
    refl = rng.integers(0, 2, ROWS_PER_MATERIAL).astype(np.int32)
    rows[:, 9:11] = rng.random((ROWS_PER_MATERIAL, 2))
    rows[:, 11:13] = rng.random((ROWS_PER_MATERIAL, 2))
    z = np.array([0.0, 0.0, 1.0])
    for i in range(96):
        ior = ior3[ch[i]]
        s = min(ior, 1.0 / ior) if ior > 0 else 0.5
        cos_c = np.sqrt(max(0.0, 1.0 - s * s))
        side = 1.0 if ior >= 1.0 else -1.0
        if i < 48:
            c = cos_c * (1.0 - 10.0 ** (-2.0 + 2.0 * i / 47.0))
        elif i < 78:
            c = min(1.0, cos_c * (1.0 + 10.0 ** (-2.0 + 2.0 * (i - 48) / 29.0)) + 1e-3)
        else:
            c = float(_ulps(cos_c, (i - 78) % 9 - 4))
            side = side if i < 87 else -side
        if i < 78:
            n, t = _frame(rng)
        else:
            n, t = z, np.array([1.0, 0.0, 0.0])
        rows[i, 0:3] = side * c * n + np.sqrt(max(0.0, 1.0 - c * c)) * t
        if i >= 78:
            rows[i, 2] = f32(side) * f32(c)
        rows[i, 3:6] = n
        rows[i, 6:9] = n
    for i in range(96, 160):
        n, t = _frame(rng)
        refract = i < 128
        k = None if (i - 96) % 32 < 15 else (i - 96) % 32 - 15 - 8
        for _ in range(64):
            cosw = rng.uniform(0.05, 1.0) * (1.0 if rng.random() < 0.5 else -1.0)
            wi = cosw * n + np.sqrt(1.0 - cosw * cosw) * t
            h = _tilted(rng, n, k)
            if not refract:
                wo = 2.0 * (wi @ h) * h - wi
                break
            ior = ior3[ch[i]]
            eta = ior if cosw > 0 else float(f32(1.0 / ior))
            disc = (wi @ h) ** 2 - 1.0 + eta * eta
            if disc < 0:
                continue
            cand = [-(wi + (-(wi @ h) + sg * np.sqrt(disc)) * h) / eta for sg in (1.0, -1.0)]
            cand = [w for w in cand if (w @ n) * cosw < 0]
            if cand:
                wo = cand[0]
                break
        else:
            wo = -wi
        rows[i, 0:3], rows[i, 3:6], rows[i, 6:9] = wi, wo, n
        refl[i] = 0 if refract else 1
    small = [f32(0.0), f32(-0.0), f32(1e-7), f32(-1e-7)]
    for i in range(160, 192):
        j = i - 160
        for col, zv in ((0, small[j % 4]), (3, small[(j // 4) % 4])):
            phi = rng.uniform(0, 2 * np.pi)
            rows[i, col:col + 3] = [np.cos(phi), np.sin(phi), 0.0]
            rows[i, col + 2] = zv
        rows[i, 6:9] = z
        refl[i] = j // 16
    u_edge = [_ulps(0.05 + k / 10.0, d) for k in range(2, 8) for d in (-1, 0, 1)]
    v_edge = [_ulps(k / 12.0, d) for k in range(0, 10) for d in (-1, 0, 1)]
    for i in range(192, 256):
        n, _ = _frame(rng)
        rows[i, 0:3] = rows[i, 3:6] = rows[i, 6:9] = n
        j = i - 192
        rows[i, 9] = u_edge[j % len(u_edge)] if j < 48 else rng.uniform(0.35, 0.65)
        rows[i, 10] = v_edge[(7 * j) % len(v_edge)] if j < 32 else rng.uniform(0.0, 0.66)
        refl[i] = 1
    return rows, ch, refl
