"""The chain scene shared by tests/test_gpu_lbvh.py and tests/test_gpu_shadow_query.py: a linear BVH of about n levels."""
import numpy as np


def chain_scene(pkg, n):
    """n triangles that all cover the square [-1, 0]^2 of their plane z = const, the k-th one reaching out to 2^(k // 3) along the
    axis k % 3 (long in x, long in y, or far away in z): every centroid has its own leading bit in the interleaved Morton code, so
    the linear BVH is one chain of about n levels, and a ray along +z through that square meets every box of it."""
    base = pkg.scenes.cornell_rc(32, 32, 1)
    tri = np.zeros(n, dtype=base.triangles.dtype)
    for k in range(n):
        L = np.float32(3.0 * 2.0 ** (k // 3 + 1))
        a = k % 3
        z = np.float32(0.01 * k) if a < 2 else L
        if a == 0:
            v = [[-1, -1, z], [L, -1, z], [-1, 1, z]]
        elif a == 1:
            v = [[-1, -1, z], [1, -1, z], [-1, L, z]]
        else:
            v = [[-1, -1, z], [3, -1, z], [-1, 3, z]]
        tri["v0"][k], tri["v1"][k], tri["v2"][k] = np.float32(v)
    obj = np.zeros(1, dtype=base.objects.dtype)
    obj["kind"], obj["material"], obj["first_tri"], obj["n_tri"] = 0, 0, 0, n
    return pkg.scenes.SceneData(triangles=tri, materials=base.materials[:1].copy(), objects=obj, background=base.background,
                                env_pixels=None, camera=base.camera, rr_rate=base.rr_rate)
