"""Pixel-centre feature rays (include/mcpt.h: mcpt_feature_opts, mcpt_centre_rays): a numpy float32 restatement of the centre ray, every
operation in the kernel's order (csrc/mcpt_kernels.hip: camera_ray_from with u = {0.5, 0.5, 0, 0}), a float64 one, and the cameras that
tests/test_centre_cpu.py and tests/test_gpu_centre.py share."""
import numpy as np

f32 = np.float32


def _scalar(v):
    return np.asarray(v).reshape(-1)[0]


def camera_consts(cam):
    """(W, H, scale, aspect) as the library's make_camera forms them: deg2rad in double from the float32 product, tan in double, each
    rounded once to float32; aspect = W / (float) H."""
    W, H = int(_scalar(cam["width"])), int(_scalar(cam["height"]))
    rad = f32(np.float64(f32(_scalar(cam["fov"])) * f32(0.5) * f32(3.141592653589793)) / 180.0)
    scale = f32(np.tan(np.float64(rad)))
    aspect = f32(W) / f32(H)
    assert scale.dtype == f32 and aspect.dtype == f32
    return W, H, scale, aspect


def _dot3(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _mat3_mul(M, v):
    return [M[0] * v[0] + (M[1] * v[1] + M[2] * v[2]), M[3] * v[0] + (M[4] * v[1] + M[5] * v[2]), M[6] * v[0] + (M[7] * v[1] + M[8] * v[2])]


def _normalized(v):
    z = _dot3(v, v)
    with np.errstate(all="ignore"):
        s = np.sqrt(z)
        return [np.where(z > 0, c / s, c) for c in v]


def centre_rays_f32(cam, pixels=None):
    """The centre rays of `pixels` (default: every pixel in order) in float32, operation by operation as the kernel: (origins[n, 3],
    dirs[n, 3]).  sin(0) = +0.f and cos(0) = 1.f are the bits the library's sincos gives at theta = 0."""
    W, H, scale, aspect = camera_consts(cam)
    m = np.arange(W * H, dtype=np.uint32) if pixels is None else np.asarray(pixels, np.uint32)
    i, j = (m % np.uint32(W)).astype(np.int32), (m // np.uint32(W)).astype(np.int32)
    u = [f32(0.5), f32(0.5), f32(0), f32(0)]
    one, two = f32(1), f32(2)
    x = (one - two * (i.astype(f32) + u[0]) / f32(W)) * aspect * scale
    y = (one - two * (j.astype(f32) + u[1]) / f32(H)) * scale
    z = np.ones_like(x)
    M = [f32(v) for v in np.asarray(cam["orientation"], f32).reshape(9)]
    eye = [f32(v) for v in np.asarray(cam["position"], f32).reshape(3)]
    if int(_scalar(cam["use_dof"])):
        fd, ap = f32(_scalar(cam["focal_distance"])), f32(_scalar(cam["aperture_radius"]))
        focal = [x * fd, y * fd, z * fd]
        r = ap * np.sqrt(u[2])
        st, ct = f32(0), f32(1)
        dx, dy = r * ct, r * st
        off = _mat3_mul(M, [dx, dy, f32(0)])
        pos = [np.full_like(x, eye[k] + off[k]) for k in range(3)]
        d = _normalized([focal[0] - dx, focal[1] - dy, focal[2] - f32(0)])
    else:
        d = _normalized([x, y, z])
        pos = [np.full_like(x, eye[k]) for k in range(3)]
    d = _mat3_mul(M, d)
    o, d = np.stack(pos, -1), np.stack(d, -1)
    assert o.dtype == f32 and d.dtype == f32
    return o, d


def centre_rays_f64(cam):
    """The pinhole ray through every pixel centre in float64 (scale and aspect: the float32 values the library uses)."""
    W, H, scale, aspect = camera_consts(cam)
    M = np.asarray(cam["orientation"], np.float64).reshape(3, 3)
    j, i = np.mgrid[0:H, 0:W]
    x = (1 - 2 * (i + 0.5) / W) * np.float64(aspect) * np.float64(scale)
    y = (1 - 2 * (j + 0.5) / H) * np.float64(scale)
    d = np.stack([x, y, np.ones_like(x)], -1).reshape(-1, 3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)) @ M.T
    o = np.broadcast_to(np.asarray(cam["position"], np.float64).reshape(3), d.shape).copy()
    return o, d


def cameras(pkg):
    """name -> (SceneData, camera): Cornell 64 x 64 without and with depth of field, chess 96 x 54 with its own depth-of-field camera."""
    cornell = pkg.scenes.cornell_demo(64, 64, 4)
    dof = pkg.scenes.make_camera(64, 64, 40, (278, 273, -800), (278, 273, 0), (0, 1, 0), use_dof=True, focal_distance=900, aperture_radius=40)
    chess = pkg.scenes.chess_scene(width=96, height=54, spp=8)
    assert int(_scalar(cornell.camera["use_dof"])) == 0 and int(_scalar(chess.camera["use_dof"])) == 1
    return {"cornell": (cornell, cornell.camera), "cornell_dof": (cornell, dof), "chess_dof": (chess, chess.camera)}


def small_camera(pkg, width, height, use_dof):
    return pkg.scenes.make_camera(width, height, 40, (278, 273, -800), (278, 273, 0), (0, 1, 0), use_dof=use_dof, focal_distance=900, aperture_radius=40)
